"""Stage K set-ups through the C API, bit for bit against what the commit before the
round-trip work at the launch ends computed (tests/golden/setup_bits.npz, recorded by
tools/record_setup_bits.py): the changes there move loads, stores and one spline builder
around and touch no arithmetic, so every byte the API hands back must stay what it was.

Per case, for every epoch: the status words (read back, and the words the finalising launch
mirrors into pinned host memory), the epoch record's scalars, every table of the set-up
(ln M, nu, the knot families, their evaluation counts), look-ups through the mass function's
two splines and normalisations, and a 64-k Stage E row per spectrum.  The large arrays are
compared by SHA-256, the status words and the deep-knot counts by value.

The C API hands out no raw view of the table block, of `search` or of the node tables; they
are covered through everything that is computed from them (the tables, the knots' values and
evaluation counts, the spectra).
"""
import hashlib
import os

import numpy
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "setup_bits.npz")

# name -> (redshifts, cosmologies, mass function, spectra, divmax)
_OTHER = {"sigma_8": 0.75, "h": 0.68, "n_scalar": 0.97}
CASES = {
    # the headline path: nothing listed, block e finalises epoch e
    "a_pmm_3": (numpy.linspace(0.0, 1.0, 3), 1, "st", ("power_mm",), None),
    # knots are listed: the finalisation goes through the arrival count, with fences
    "b_tinker_pgm_2": (numpy.array([0.2, 0.9]), 1, "tinker", ("power_gm",), None),
    # the one-epoch launch shapes
    "c_pmm_1": (numpy.array([0.5]), 1, "st", ("power_mm",), None),
    # two cosmology slots: the slot is read per epoch
    "d_pmm_9_two_cosmologies": (numpy.linspace(0.0, 1.6, 9), 2, "st", ("power_mm",), None),
    # the two-phase probe
    "e_pmm_130": (numpy.linspace(0.0, 2.0, 130), 1, "st", ("power_mm",), None),
    # the literal normalisation branch, divmax within two levels of the node tables
    "f_pmm_3_divmax12": (numpy.linspace(0.0, 1.0, 3), 1, "st", ("power_mm",), 12),
}
_TABLES = {"power_mm": ("h_m", "pp_mm"), "power_gm": ("h_m", "h_g", "pp_gm")}
_EVALS = ("nu_of_mass", "ln_mass_of_nu", "f_nu", "bias_nu")


def _sha(a):
    return hashlib.sha256(numpy.ascontiguousarray(a).tobytes()).hexdigest()


def measure(name):
    """Run case `name` on a fresh context; {key: numpy array or str}."""
    from chomp_amd import _lib, cosmology, defaults, grid
    z, n_cosmo, mf, spectra, divmax = CASES[name]
    z = numpy.ascontiguousarray(z, dtype=numpy.float64)
    n = z.size
    precision = dict(defaults.default_precision)
    if divmax is not None:
        precision["divmax"] = divmax
    ctx = _lib.Context(_lib.make_config(defaults.default_limits, precision),
                       device=_lib.current_device())
    cosmos = [defaults.default_cosmo_dict] * n
    if n_cosmo == 2:
        cosmos = [defaults.default_cosmo_dict if i < 5 else dict(defaults.default_cosmo_dict, **_OTHER)
                  for i in range(n)]
    c = ctx.pack_cosmo(cosmos, n)
    h = ctx.pack_halo(defaults.default_halo_dict, n)
    hod = ctx.pack_hod(grid._hod_object(defaults.default_hod_dict), n)
    need = 0
    for s in spectra:
        need |= grid._WHICH[s][1]
    ctx.epochs_set(c, z, **cosmology._de_kw(c))
    ctx.stage_k(h, _lib.MF_TINKER if mf == "tinker" else _lib.MF_ST, h, hod, need)
    ctx.status_post()
    out = {"status_posted": ctx.status_wait(0, n).astype(numpy.uint32)}
    out["status"] = ctx.status(0, n).astype(numpy.uint32)
    out["deep_stats"] = numpy.array(ctx.deep_stats(), dtype=numpy.int64)
    sc = numpy.array([[ctx.scalars(e)[k] for k in _lib.SC] for e in range(n)])
    out["scalars_sha"] = _sha(sc)
    out["scalars_epoch0"] = sc[0]
    tables = ["ln_mass", "nu", "levels"]
    for s in spectra:
        tables += [t for t in _TABLES[s] if t not in tables]
    for t in tables:
        out["table_" + t + "_sha"] = _sha(numpy.stack([ctx.table(t, e) for e in range(n)]))
    lnm = ctx.table("ln_mass", 0)
    nu = ctx.table("nu", 0)
    mass = numpy.exp(numpy.linspace(lnm[1], lnm[-2], 16))
    nus = numpy.linspace(1.01 * nu[1], 0.99 * nu[-2], 16)
    for what in _EVALS:
        x = mass if what == "nu_of_mass" else nus
        out["eval_" + what + "_sha"] = _sha(numpy.stack([ctx.eval(what, x, e) for e in range(n)]))
    k = numpy.logspace(-3, 2, 64)
    for s in ("linear_power",) + tuple(spectra):
        out["power_" + s + "_sha"] = _sha(ctx.power(grid._WHICH[s][0], k, 0, n))
    ctx.close()
    return out


def check_shape(name, got):
    """What a case must show for it to take the path it is there for."""
    fast, literal = (int(v) for v in got["deep_stats"])
    if name.startswith("b_"):
        assert fast + literal > 0, "no knot was listed: the arrival path did not run"
    else:
        assert fast + literal == 0, "a knot was listed on a P_mm set-up"
    assert numpy.array_equal(got["status"], got["status_posted"])


@pytest.fixture(scope="module")
def golden():
    with numpy.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_setup_bits(name, golden):
    got = measure(name)
    check_shape(name, got)
    keys = sorted(k[len(name) + 1:] for k in golden if k.startswith(name + "/"))
    assert keys == sorted(got), (keys, sorted(got))
    for key in keys:
        want = golden[name + "/" + key]
        if key.endswith("_sha"):
            assert str(want) == got[key], (name, key)
        else:
            assert want.dtype == got[key].dtype and want.tobytes() == got[key].tobytes(), (
                name, key, want, got[key])
