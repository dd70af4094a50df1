"""PerturbationTheory on the MI355X (pytest -m gpu): every form against the reference's own
numbers (G23, tests/golden/make_golden_pt.py) and against the numpy restatement of
test_perturbation_cpu fed with the device's SingleEpoch.linear_power; the edge cases exactly;
epoch batches, *_many and torch input against single calls bit for bit; a launch of 2^20 + 13
configurations."""
import numpy
import pytest

from conftest import load_golden
from params import c_dict_2
from test_perturbation_cpu import PT_FORMS, close_or_same, restate

pytestmark = pytest.mark.gpu

CASES = (("def_", None, 0.0), ("def_", None, 0.5), ("c2_", c_dict_2, 0.0), ("c2_", c_dict_2, 0.5))


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def g():
    return load_golden("g23_perturbation")


def _pt(cd, z):
    from chomp_amd import cosmology, perturbation_spectra
    return perturbation_spectra.PerturbationTheory(z, cosmology.SingleEpoch(z, cd))


def _single(pt, form, row):
    """The reference's single-configuration method on one row of arguments."""
    fn = getattr(pt, form)
    if form in ("Fs2", "Fs3", "F3", "Fs3_BCGS", "bispectrum", "trispectrum"):
        return fn(*[row[3 * j:3 * j + 3] for j in range(row.size // 3)])
    return fn(*row)


@pytest.mark.parametrize("tag,cd,z", CASES)
@pytest.mark.parametrize("form", PT_FORMS)
def test_form_against_reference_and_restatement(lib, g, form, tag, cd, z):
    pt = _pt(cd, z)
    args = g["pt_args_" + form]
    got = pt.cosmo._dev().pt_eval(form, args, 0, 1)[0]
    want, scale = restate(form, args, pt.cosmo.linear_power)
    close_or_same(got, want, scale, 1e-13)
    close_or_same(got, g[tag + "z%03d_" % int(round(100 * z)) + form], scale, 1e-6)
    # the reference's method surface: one configuration per call, the same bits
    for i in (0, 7, args.shape[0] - 1):
        v = _single(pt, form, args[i])
        assert numpy.array_equal(v, got[i], equal_nan=True), (i, v, got[i])


def test_edge_cases_exactly(lib):
    pt = _pt(None, 0.0)
    z, k = numpy.zeros(3), numpy.array([0.1, 0.05, -0.02])
    assert pt.Fs2(z, k) == 5. / 7. and pt.Fs2(k, 5e-9 * k / numpy.sqrt(k @ k)) == 5. / 7.
    assert pt.Fs2_len(5e-9, 0.1, 0.3) == 5. / 7. and pt.Fs2_len(0.1, 0.0, 0.3) == 5. / 7.
    assert pt.cosmo.linear_power(numpy.array([1e-17]))[0] == 1e-16
    # bispectrum_len with k3 < 1e-16: P(k3) = 1e-16 exactly, Fs2_len = 5/7
    p1, p2 = pt.cosmo.linear_power(numpy.array([0.1, 0.2]))
    f12 = pt.Fs2_len(0.1, 0.2, 0.3)
    want = 2. * ((f12 * p1 * p2 + 5. / 7. * p1 * 1e-16) + 5. / 7. * p2 * 1e-16)
    assert pt.bispectrum_len(0.1, 0.2, 1e-17, 0.3, 0.4, 0.5) == want
    # Fs3 with a zero vector: c4 divides by zero (inf or NaN as numpy gives)
    assert not numpy.isfinite(pt.Fs3(z, k, 2 * k))
    # k1 + k2 = 0: P_lin(0) = 1e-16, the trispectrum stays finite
    k3, k4 = numpy.array([0.03, -0.1, 0.2]), numpy.array([-0.2, 0.01, 0.05])
    assert numpy.isfinite(pt.trispectrum(k, -k, k3, k4))
    # mu = 1, k1 = k2: |k1 - k2| = 0 < 1e-8 in Fs2_kdiff's Fs2_len (its z is 0/0, not used)
    assert pt.Fs2_kdiff(0.1, 0.1, 1.0) == 5. / 7.


@pytest.mark.parametrize("form", ("bispectrum", "trispectrum", "trispectrum_parallelogram",
                                  "Fs3"))
def test_epoch_batch_equals_single_epochs(lib, g, form):
    from chomp_amd import cosmology, defaults
    ctx = cosmology._context()
    zs = numpy.array([0.0, 0.25, 0.5, 1.0, 2.0])
    ctx.epochs_set(defaults.default_cosmo_dict, zs)
    args = g["pt_args_" + form]
    whole = ctx.pt_eval(form, args, 0, zs.size)
    for i in range(zs.size):
        assert numpy.array_equal(whole[i], ctx.pt_eval(form, args, i, 1)[0], equal_nan=True)
    mid = ctx.pt_eval(form, args, 1, 3)
    assert numpy.array_equal(mid, whole[1:4], equal_nan=True)
    # epoch i of the batch is the SingleEpoch at that redshift
    pt = _pt(None, 0.5)
    assert numpy.array_equal(whole[2], pt.cosmo._dev().pt_eval(form, args, 0, 1)[0],
                             equal_nan=True)


def test_many_equal_single_calls(lib, g):
    pt = _pt(None, 0.5)
    b = g["pt_args_bispectrum"][:64].reshape(-1, 3, 3)
    got = pt.bispectrum_many(b[:, 0], b[:, 1], b[:, 2])
    assert got.shape == (64,)
    for i in range(64):
        assert got[i] == pt.bispectrum(b[i, 0], b[i, 1], b[i, 2])
    t = g["pt_args_trispectrum"][:64].reshape(-1, 4, 3)
    got = pt.trispectrum_many(t[:, 0], t[:, 1], t[:, 2], t[:, 3])
    for i in range(64):
        assert numpy.array_equal(got[i], pt.trispectrum(*t[i]), equal_nan=True)


def test_torch_input_equals_host(lib, g):
    import torch
    pt = _pt(None, 0.0)
    ctx = pt.cosmo._dev()
    for form in PT_FORMS:
        args = g["pt_args_" + form]
        host = ctx.pt_eval(form, args, 0, 1)
        dev = ctx.pt_eval(form, torch.from_numpy(numpy.ascontiguousarray(args)).cuda(), 0, 1)
        assert numpy.array_equal(dev.cpu().numpy(), host, equal_nan=True), form
    t = torch.from_numpy(g["pt_args_trispectrum"][:100].reshape(-1, 4, 3).copy()).cuda()
    got = pt.trispectrum_many(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(),
                              t[:, 3].contiguous())
    want = pt.trispectrum_many(*[t[:, j].cpu().numpy() for j in range(4)])
    assert numpy.array_equal(got.cpu().numpy(), want, equal_nan=True)


@pytest.mark.parametrize("form", ("bispectrum_len", "trispectrum"))
def test_large_launch(lib, form):
    pt = _pt(None, 0.5)
    ctx = pt.cosmo._dev()
    n = (1 << 20) + 13
    rng = numpy.random.default_rng(5)
    if form == "bispectrum_len":
        args = numpy.concatenate([10.0 ** rng.uniform(-3, 1, (n, 3)), rng.uniform(-1, 1, (n, 3))],
                                 axis=1)
    else:
        args = rng.normal(size=(n, 12)) * 0.3
    got = ctx.pt_eval(form, args, 0, 1)[0]
    assert got.shape == (n,)
    pick = numpy.concatenate([numpy.arange(512), rng.integers(0, n, 2048), numpy.arange(n - 600, n)])
    assert numpy.array_equal(got[pick], ctx.pt_eval(form, args[pick], 0, 1)[0])
    want, scale = restate(form, args[pick], pt.cosmo.linear_power)
    close_or_same(got[pick], want, scale, 1e-13)
