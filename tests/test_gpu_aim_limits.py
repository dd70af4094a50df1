"""The mass limits through the C ABI with the aim of the search solved for (one-pass ln S table,
inverse interpolation in plan_side; pytest -m gpu): ln M_min and ln M_max `==` the oracle's
walk, no status bit, in every launch shape that aims -- eight epochs in one launch, one epoch
alone (k_nu_table<., 4> and the single-epoch probes), and 130 epochs (probing and certifying
phases, single-wavefront probes: the same plan_side on a block of 64).

Every side of these inputs is CERTIFIED BY ITS PROBES, so that no assertion here can pass through
the exact-search fallback: a walk of j steps is settled by the probes at candidates j - 2 .. j + 1
that exist (index > 0), i.e. min(4, j + 1) integrals, a side that stays at its starting mass by
none -- or by one, the start itself, where the start lies within the plan's margin of a band
edge (z = 1.29, mass_max) -- and n_search, the integrals of both sides, is exactly their sum (at
most 4 a side; the fallback adds at least one).  The same holds for the parent of this change (verified: this file
passes unchanged on it), so the evaluation counts did not move."""
import numpy
import pytest

pytestmark = pytest.mark.gpu

Z8 = numpy.linspace(0.0, 1.5, 8)
SOAK96 = dict(omega_m0=0.282801919784524, omega_b0=0.04606049457071416,
              omega_l0=0.717113386337925, h=0.615423691856908, sigma_8=0.7320155736315984,
              n_scalar=0.9301320614204301)
SOAK96_Z = 0.9637352201784997
LN_105 = numpy.log(1.05)
EDGE_MARGIN = 0.00995033085          # plan_side's ln(1 + 1e-2)


def _walk(z, cosmo=None):
    """The oracle's limits at z and the integrals the probes certify them with."""
    from oracle import chomp_oracle as o
    e = o.epoch(cosmo, float(z))
    lo, hi, _ = o.mass_limits(e)
    n_eval = 0
    for start, band, limit in ((1e9, 0.1, lo), (1e16, 50.0, hi)):
        j = round(abs(limit - numpy.log(start)) / LN_105)
        # the starting mass within plan_side's margin (1 %) of a band edge: the probes are
        # candidates 0 .. 3, the start decides exactly and is counted
        off = min(abs(numpy.log(o.nu_m(e, start) / (band * f))) for f in (0.95, 1.05))
        assert abs(off - EDGE_MARGIN) > 1e-3, "an input on the margin's own edge: choose another"
        if off < EDGE_MARGIN:
            n_eval += 1 + (3 if j > 0 else 0)
            assert j == 0 or j <= 3, "an edge start whose walk the four probes do not cover"
        elif j > 0:
            n_eval += min(4, j + 1)
    return lo, hi, n_eval


@pytest.fixture(scope="module")
def walks8():
    return [_walk(z) for z in Z8]


def _check(hg, i, want):
    lo, hi, n_eval = want
    sc = hg.ctx.scalars(i)
    print(i, sc["ln_mass_min"], sc["ln_mass_max"], int(sc["n_search"]), n_eval)
    assert hg.status()[i] == 0
    assert sc["ln_mass_min"] == lo and sc["ln_mass_max"] == hi, (i, sc["ln_mass_min"] - lo,
                                                                sc["ln_mass_max"] - hi)
    assert int(sc["n_search"]) == n_eval, (i, int(sc["n_search"]), n_eval)


def _grid(z, cosmo=None):
    from chomp_amd import grid
    z = numpy.atleast_1d(numpy.asarray(z, dtype=float))
    hg = grid.HaloGrid(z) if cosmo is None else grid.HaloGrid(z, cosmo_dict=[cosmo] * z.size)
    hg.setup("power_mm")
    return hg


def test_eight_epochs(walks8):
    hg = _grid(Z8)
    for i in range(Z8.size):
        _check(hg, i, walks8[i])


def test_soak_case_96():
    from oracle import chomp_oracle as o
    cd = dict(o.default_cosmo_dict, **SOAK96)
    _check(_grid([SOAK96_Z], cd), 0, _walk(SOAK96_Z, cd))


@pytest.mark.parametrize("i", (0, 3, 7))
def test_single_epoch(walks8, i):
    _check(_grid([Z8[i]]), 0, walks8[i])


def test_130_epochs(walks8):
    """The eight redshifts spread among 122 others: the two-launch shape."""
    z = numpy.linspace(0.005, 1.495, 130)
    where = numpy.arange(8) * 18 + 1
    z[where] = Z8
    hg = _grid(z)
    for i, w in zip(where, walks8):
        _check(hg, int(i), w)
    st = hg.status()
    assert not numpy.any(st[:130])
    assert max(int(hg.ctx.scalars(i)["n_search"]) for i in range(130)) <= 8
