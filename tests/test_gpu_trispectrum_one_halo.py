"""HaloTrispectrumOneHalo on the MI355X (pytest -m gpu): the I_0^4 tables, their Romberg levels,
the spline and the quadruple integrals against the reference's own numbers (G24,
tests/golden/make_golden_tri1h.py) and the oracle's levels; the table against the quadruple
path; an epoch batch against single epochs; torch input; the stale and rebuilt sequences."""
import numpy
import pytest

from conftest import load_golden, rel_err
from params import c_dict_2, h_dict_2
from test_trispectrum_one_halo_cpu import TAGS, full, oracle_tri

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def g():
    return load_golden("g24_trispectrum_one_halo")


def make(tag):
    from chomp_amd import cosmology, hod, mass_function
    from chomp_amd.halo_trispectrum import HaloTrispectrumOneHalo as HT
    if tag in ("z000_", "z050_"):
        return HT(0.0 if tag == "z000_" else 0.5)
    if tag in ("gmmm_", "ggmm_", "gggm_", "gggg_"):
        return HT(0.3, power_spec="power_" + tag[:4], input_hod=hod.HODZheng())
    if tag == "mand_":
        return HT(0.3, power_spec="power_gggg",
                  input_hod=hod.HODMandelbaum({"log_M_0": 12.14, "w": 1.0}))
    if tag == "alt_":
        cosmo = cosmology.SingleEpoch(0.3, c_dict_2)
        return HT(0.3, cosmo, mass_function.TinkerMassFunction(0.3, cosmo, h_dict_2), None,
                  h_dict_2)
    cosmo = cosmology.SingleEpoch(0.2)
    return HT(0.2, cosmo, mass_function.MassFunctionSecondOrder(0.2, cosmo))


def scal(h, pairs):
    return numpy.array([numpy.asarray(h.trispectrum_parallelogram(a, b)).ravel()[0]
                        for a, b in pairs])


@pytest.mark.parametrize("tag", TAGS)
def test_g24_case(lib, g, tag):
    h = make(tag)
    h.trispectrum_parallelogram(1.0, 1.0)
    assert h._initialized_i_0_4 is True
    assert rel_err(h._i_0_4_array, full(g[tag + "table"])) < 1e-8
    o_tab, o_lev, o_q, o_qlev = oracle_tri(tag)
    bad = numpy.argwhere(h._i_0_4_levels != o_lev)
    assert bad.size == 0, "pairs whose Romberg level differs from the oracle's: %s" % bad.tolist()
    q, qlev = h._sync(0).tri1h_quad(h._moment(), g["quads"], 0, levels=True)
    assert rel_err(q, g[tag + "quad"]) < 1e-8
    assert numpy.array_equal(qlev, o_qlev)
    assert rel_err(h.i_0_4_many(g["quads"]), g[tag + "quad"]) < 1e-8
    k = g["quads"][3]
    assert abs(h.i_0_4(*k) / g[tag + "quad"][3] - 1) < 1e-8
    assert abs(h.trispectrum(*k) / g[tag + "quad"][3] - 1) < 1e-8
    if tag + "scal" in g.files:
        got = scal(h, g["pairs"])
        ref = g[tag + "scal"]
        assert numpy.array_equal(got == 0.0, ref == 0.0)
        nz = ref != 0.0
        assert rel_err(got[nz], ref[nz]) < 1e-7
    assert h._tri_ctx.status(0, 1)[0] == 0
    assert h._sync(0).status(0, 1)[0] == 0


def test_array_calls_and_shapes(lib, g):
    h = make("z000_")
    for name in ("arr_", "arr_col_", "arr_row_", "arr_rev_"):
        a, b = g[name + "a"], g[name + "b"]
        a = a if a.size > 1 else float(a[0])
        b = b if b.size > 1 else float(b[0])
        got = numpy.asarray(h.trispectrum_parallelogram(a, b))
        ref = g[name + "out"]
        assert got.shape == tuple(g[name + "shape"])
        assert numpy.array_equal(got == 0.0, ref == 0.0)
        assert rel_err(got[ref != 0.0], ref[ref != 0.0]) < 1e-7
    assert h.trispectrum_parallelogram(0.5, 2.0).shape == (1, 1)


def test_table_against_quadruple_path(lib):
    h = make("z000_")
    h.trispectrum_parallelogram(1.0, 1.0)
    kk = numpy.exp(h._ln_k_array)
    i, j = numpy.meshgrid(numpy.arange(50), numpy.arange(50), indexing="ij")
    k = numpy.stack([kk[i.ravel()], kk[i.ravel()], kk[j.ravel()], kk[j.ravel()]], axis=1)
    q, lev = h._sync(0).tri1h_quad(0, k, 0, levels=True)
    assert rel_err(h._i_0_4_array.ravel(), q) < 1e-12
    assert numpy.array_equal(h._i_0_4_levels.ravel(), lev)


def test_epoch_batch_equals_single_epochs(lib):
    from chomp_amd import cosmology, defaults, hod
    z = numpy.linspace(0.0, 1.4, 8)
    prof = defaults.default_halo_dict
    batch = cosmology._context()
    batch.epochs_set(defaults.default_cosmo_dict, z)
    batch.stage_k(prof, lib.MF_ST, prof, hod.HODZheng(), 0)
    tab, lev = batch.tri1h_setup(4, 0, 8, copy_out=True)
    ln_a = numpy.log(numpy.array([2e-3, 0.3, 1.0, 40.0]))
    ln_b = numpy.log(numpy.array([0.05, 0.3, 7.0, 99.0]))
    for e in range(8):
        one = cosmology._context()
        one.epochs_set(defaults.default_cosmo_dict, z[e:e + 1])
        one.stage_k(prof, lib.MF_ST, prof, hod.HODZheng(), 0)
        t1, l1 = one.tri1h_setup(4, 0, 1, copy_out=True)
        assert numpy.array_equal(t1[0], tab[e]) and numpy.array_equal(l1[0], lev[e])
        assert numpy.array_equal(one.tri1h_eval(ln_a, ln_b, 0), batch.tri1h_eval(ln_a, ln_b, e))
    assert numpy.all(batch.status(0, 8) == 0)


def test_torch_input(lib, g):
    import torch
    h = make("gggm_")
    kt = torch.tensor(g["quads"], dtype=torch.float64, device="cuda")
    got = h.i_0_4_many(kt)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert numpy.array_equal(got.cpu().numpy(), h.i_0_4_many(g["quads"]))


def test_stale_and_rebuilt_sequences(lib, g):
    from chomp_amd.halo_trispectrum import HaloTrispectrumOneHalo as HT
    from chomp_amd.perturbation_spectra import PerturbationTheory
    h = HT(0.0)
    h.trispectrum_parallelogram(0.5, 2.0)
    with pytest.raises(AttributeError):
        h.set_redshift(0.5)
    assert h._redshift == 0.5 and h._initialized_i_0_4 is True
    got = scal(h, g["pairs"])
    ref = g["stale_scal"]
    assert numpy.array_equal(got == 0.0, ref == 0.0)
    assert rel_err(got[ref != 0.0], ref[ref != 0.0]) < 1e-7
    assert rel_err(h.i_0_4_many(g["quads"][:8]), g["stale_quad"]) < 1e-8
    h = HT(0.0, perturbation=PerturbationTheory(0.0))
    h.trispectrum_parallelogram(0.5, 2.0)
    h.set_redshift(0.5)
    assert h._initialized_i_0_4 is False
    got = scal(h, g["pairs"])
    ref = g["rebuilt_scal"]
    assert numpy.array_equal(got == 0.0, ref == 0.0)
    assert rel_err(got[ref != 0.0], ref[ref != 0.0]) < 1e-7
    assert rel_err(h._i_0_4_array, full(g["z050_table"])) < 1e-8


def test_scope_and_state_errors(lib):
    from chomp_amd import cosmology, defaults, hod
    from chomp_amd.halo_trispectrum import HaloTrispectrumOneHalo as HT
    with pytest.raises(lib.ChompScopeError):
        HT(0.0, input_hod=hod.HODPoisson())
    with pytest.raises(lib.ChompScopeError):
        HT(0.0, halo_dict=dict(defaults.default_halo_dict, alpha=-1.5))
    ctx = cosmology._context()
    ctx.epochs_set(defaults.default_cosmo_dict, [0.0])
    with pytest.raises(lib.ChompError):            # no halo set-up yet
        ctx.tri1h_setup(0)
    ctx.stage_k(defaults.default_halo_dict, lib.MF_ST, defaults.default_halo_dict,
                hod.HODZheng(), 0)
    with pytest.raises(lib.ChompError):            # no table yet
        ctx.tri1h_eval([0.0], [0.0], 0)
    with pytest.raises(ValueError):
        ctx.tri1h_setup(7)
