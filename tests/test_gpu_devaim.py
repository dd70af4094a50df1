"""The AIM of the mass-limit search AS COMPILED FOR THE DEVICE (tests/devcheck/devaim.hip, the
product's compiler flags): the coarse ln S(R) table k_sigma_nodes<false, 1> fills in one pass
over the level-10 Romberg grid, and plan_side's inverse interpolation of the step at which the
estimated walk stops.

The aim decides nothing -- the probes certify, and a wrong aim only costs the exact search -- but
a poor one would cost that search on every set-up, so both halves are held to what plan_side
assumes of them:

* ln S: every one of the 48 table values within 1e-4 (relative, in S) of the same integral at the
  reference's tolerance (romberg1 on SigmaIntegrandT, cosmo_precision, divmax), the estimate error
  plan_side's comment states against its safety margin of 1e-2.  The adaptive rule the one pass
  replaced (rtol 1e-5, cap 10) is evaluated beside it and printed: it meets the same bound on the
  three cosmologies (measured: see test_lns_one_pass).
* the crossing: for WMAP7 and two cosmologies jittered by 2 % in Omega_m and sigma_8, at
  z in {0, 0.5, 0.96, 1.5} and on both sides -- 24 cases, one block each, with blocks of 256 and
  of 64 threads -- the plan found by inverse interpolation is the plan of the two-round search
  over all candidates: ok, direction, index, edge flag.  On these inputs the inverse
  interpolation must check out by itself (searched == 0 wherever a walk is planned): the test
  cannot pass through the fallback.  The jitter upwards puts the starting mass of the mass_max
  side at z = 1.5 on the lower band edge (nu(1e16) = 47.5 (1 - 3.8e-3) by the oracle).  With the
  default k limits no walk at z <= 1.5 leaves the table (it reaches down to R_a / 20 by design),
  so the off-table exits are taken on a table cut short by k_min: a walk that leaves it
  (k_min = 0.009: the table ends at R = 33.3 Mpc/h, 1e16 M_sun starts at 31.7) and a starting
  mass outside it (k_min = 0.012).  There both routines must refuse alike (ok == 0).
"""
import numpy
import pytest

import devcheck_build as dcb
from devcheck_build import call, ptr
from oracle import chomp_oracle as o
from chomp_amd import defaults

pytestmark = pytest.mark.gpu

_i, _p = dcb._i, dcb._p
dcb.HARNESSES.setdefault("devaim", dcb.Harness("devaim"))
dcb.ALL_ENTRY_POINTS.setdefault("devaim", {
    "da_sgrid": [], "da_plan_out": [],
    "da_lns": [_p, _p, _i, _p],
    "da_plan": [_p, _p, _i, _p, _i, _i, _p],
})
dcb.VOID.setdefault("devaim", ())

COSMO_KEYS = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8",
              "n_scalar")
REDSHIFTS = (0.0, 0.5, 0.96, 1.5)


def _jitter(f_m, f_s):
    c = dict(o.default_cosmo_dict)
    c["omega_m0"] = o.default_cosmo_dict["omega_m0"] * f_m
    c["omega_l0"] = 1.0 - c["omega_m0"] - c["omega_r0"]          # (flat, as WMAP7 is)
    c["sigma_8"] = o.default_cosmo_dict["sigma_8"] * f_s
    return c


COSMOS = {"wmap7": dict(o.default_cosmo_dict), "minus": _jitter(0.98, 0.98),
          "plus": _jitter(1.02, 1.02)}
EDGE = ("plus", 1.5, 1)           # (cosmology, z, side) whose starting mass sits on a band edge


def _cosmo(c):
    return numpy.array([float(c[k]) for k in COSMO_KEYS])


def _limits(k_min=None):
    lim, prec = defaults.default_limits, defaults.default_precision
    return numpy.array([lim["k_min"] if k_min is None else k_min, lim["k_max"],
                        prec["cosmo_precision"], prec["global_precision"]]), int(prec["divmax"])


@pytest.fixture(scope="module")
def da():
    return dcb.load("devaim")


def _plans(L, cosmo, threads, k_min=None):
    lim, divmax = _limits(k_min)
    z = numpy.array(REDSHIFTS)
    w = L.da_plan_out()
    out = numpy.empty((z.size, 2, w))
    call(L, "da_plan", ptr(_cosmo(cosmo)), ptr(lim), divmax, ptr(z), z.size, threads, ptr(out))
    return out


@pytest.mark.parametrize("name", sorted(COSMOS))
def test_lns_one_pass(da, name):
    """Measured on the MI355X (max over the 48 points, relative in S):
    one pass 3.7e-6 / 4.1e-6 / 3.9e-6 (at R = 256 Mpc/h, where 2^10 panels end), adaptive rule
    4.1e-5 / 4.2e-5 / 4.1e-5 (at R = 2.1) for minus / plus / wmap7."""
    lim, divmax = _limits()
    n = da.da_sgrid()
    out = numpy.empty(4 * n)
    call(da, "da_lns", ptr(_cosmo(COSMOS[name])), ptr(lim), divmax, ptr(out))
    one, ref, ada, ln_r = out[:n], out[n:2 * n], out[2 * n:3 * n], out[3 * n:]
    assert numpy.all(numpy.isfinite(out))
    err_one = numpy.abs(numpy.expm1(one - ref))
    err_ada = numpy.abs(numpy.expm1(ada - ref))
    print("%s: ln S one pass max %.3g (R = %.3g), adaptive rule max %.3g (R = %.3g)"
          % (name, err_one.max(), numpy.exp(ln_r[err_one.argmax()]), err_ada.max(),
             numpy.exp(ln_r[err_ada.argmax()])))
    assert err_one.max() <= 1e-4


@pytest.mark.parametrize("threads", (256, 64))
@pytest.mark.parametrize("name", sorted(COSMOS))
def test_crossing_is_the_search(da, name, threads):
    out = _plans(da, COSMOS[name], threads)
    for iz, z in enumerate(REDSHIFTS):
        for side in (0, 1):
            inv, two = out[iz, side, 0:6], out[iz, side, 6:12]
            print(name, threads, z, side, "inverse", inv, "search", two)
            assert out[iz, side, 12] == 0                       # every thread the same plan
            assert two[4] == (1.0 if (two[1] != 0 and not two[3]) else 0.0)
            # ok, dir, j, at_edge, and the estimate at the start (the same arithmetic: bits)
            assert numpy.array_equal(inv[[0, 1, 2, 3, 5]], two[[0, 1, 2, 3, 5]])
            assert inv[0] == 1.0                                # planned, not refused
            assert inv[4] == 0.0                                # ... and not by the fallback
            if (name, z, side) == EDGE:
                assert inv[3] == 1.0 and inv[2] == 2.0
            else:
                assert inv[3] == 0.0
    # the plans are the oracle's walks: every mass_min side walks down, by the oracle's steps
    for iz, z in enumerate(REDSHIFTS):
        lo, hi, _ = o.mass_limits(o.epoch(COSMOS[name], z))
        steps = round((numpy.log(1e9) - lo) / numpy.log(1.05))
        assert out[iz, 0, 1] == -1.0 and out[iz, 0, 2] == steps, (z, out[iz, 0, :3], steps)


@pytest.mark.parametrize("threads", (256, 64))
@pytest.mark.parametrize("k_min,leaves", ((0.009, True), (0.012, False)))
def test_off_table_exits(da, k_min, leaves, threads):
    """mass_max side, z = 0 (nu(1e16) = 40: the walk goes up).  leaves: the walk leaves the ln S
    table (the estimate at the start is finite, a direction is set, no candidate is accepted);
    not leaves: the starting mass itself is outside (the estimate at the start is NaN)."""
    out = _plans(da, COSMOS["wmap7"], threads, k_min=k_min)
    inv, two = out[0, 1, 0:6], out[0, 1, 6:12]
    print(k_min, threads, "inverse", inv, "search", two)
    assert out[0, 1, 12] == 0
    assert inv[0] == 0.0 and two[0] == 0.0
    assert numpy.array_equal(inv[[0, 1, 2, 3]], two[[0, 1, 2, 3]])
    if leaves:
        assert numpy.isfinite(inv[5]) and inv[5] == two[5] and inv[1] == 1.0
        assert inv[4] == 1.0 and two[4] == 1.0                  # both went through the search
    else:
        assert numpy.isnan(inv[5]) and numpy.isnan(two[5]) and inv[1] == 0.0
