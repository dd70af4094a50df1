"""What the five batched projections refuse -- chomp_wtheta_epochs, chomp_wtheta_sets,
chomp_xi3d_epochs, chomp_cell_epochs, chomp_cell_sets -- by exception class and FULL message, and
which refusal comes first when two apply.  The texts are literals, one table per entry point: the
calls share their refusals' code, and a shared message that named the wrong call or pointed to the
wrong single-epoch call would still hold the substrings the other tests match.

Every case returns before a kernel: nothing is launched beyond the fixtures' set-ups and the one
valid call that follows each table (a refusal leaves nothing behind)."""
import copy

import numpy
import pytest

from conftest import load_golden
from test_gpu_wtheta_cosmologies import _Grid, _cosmos, _kernel, _single_setup

pytestmark = pytest.mark.gpu

# three abscissae: theta (radians), r (Mpc/h), l
X = {"wtheta": numpy.array([0.001, 0.004, 0.02]), "xi3d": numpy.array([0.5, 3.0, 20.0]),
     "cell": numpy.array([20.0, 200.0, 2000.0])}
K = (0.001, 10.0)
BAD_K = (0.0, 100.0)
STATE = " (code -3)"                         # (how _lib words CHOMP_ERR_STATE)


@pytest.fixture(scope="module")
def g34():
    import torch
    assert torch.cuda.is_available()
    return load_golden("g34_wtheta_cosmologies")


@pytest.fixture(scope="module")
def full(g34):
    """Two power_gg epochs, a two-set kernel_setup_sets and (for the *_epochs calls) a
    kernel_setup on one context."""
    G = _Grid(_cosmos(g34)[:2], "power_gg")
    _single_setup(G.ctx, G.kern, G.cosmos[0])
    return G


@pytest.fixture(scope="module")
def proj_only(g34):
    """kernel_setup only: no sets, no epochs."""
    from chomp_amd import cosmology
    ctx = cosmology._context()
    _single_setup(ctx, _kernel(), _cosmos(g34)[0])
    return ctx


@pytest.fixture(scope="module")
def wiggle_sets(g34):
    """The wiggle transfer function and a two-set kernel_setup_sets.  (A context of its own: the
    *_sets calls look at the sets first, and the switch drops a context's epochs.)"""
    from chomp_amd import cosmology
    ctx = cosmology._context()
    ctx.set_transfer(True)
    _kernel()._setup_sets_on(ctx, _cosmos(g34)[:2])
    return ctx


def _bare():
    """A fresh context: neither epochs nor a projection set-up (nothing is launched)."""
    from chomp_amd import cosmology
    return cosmology._context()


def _call(ctx, name, which, n_epoch, D, k=K, epoch0=0):
    x = X[name.split("_")[0]]
    if name == "wtheta_epochs" or name == "wtheta_sets":
        return getattr(ctx, name)(which, epoch0, n_epoch, k[0], k[1], D, x)
    if name == "xi3d_epochs":
        return ctx.xi3d_epochs(which, epoch0, n_epoch, k[0], k[1], x)
    return getattr(ctx, name)(which, epoch0, n_epoch, D, x)


def _too_large(ctx, name, D):
    """n * n_epoch beyond 2^31 - 1 straight through the C entry point (the Python layer would
    allocate the output first); it returns at its second check, before any array is touched."""
    x, out = X[name.split("_")[0]], numpy.empty(3)
    Dp = D.ctypes.data if isinstance(D, numpy.ndarray) else D
    pre = {"wtheta_epochs": (K[0], K[1], Dp), "wtheta_sets": (K[0], K[1], Dp), "xi3d_epochs": K,
           "cell_epochs": (Dp,), "cell_sets": (Dp,)}[name]
    from chomp_amd import _lib
    ctx._check(getattr(ctx._L, "chomp_" + name)(ctx._h, _lib.P_GG, 0, 1 << 30, *pre, x.ctypes.data,
                                                3, out.ctypes.data, _lib.HOST))


def _refused(cls, text, fn, *args, **kws):
    with pytest.raises(cls) as info:
        fn(*args, **kws)
    assert type(info.value) is cls and str(info.value) == text, (str(info.value), text)


def _with_precision(ctx, fn, *args):
    from chomp_amd import _lib
    ctx.set_precision(_lib.PREC_F32_EVAL)
    try:
        return fn(*args)
    finally:
        ctx.set_precision(_lib.PREC_F64)


def _with_wiggle(ctx, fn, *args):
    """(only on contexts without epochs: the switch drops them)"""
    ctx.set_transfer(True)
    try:
        return fn(*args)
    finally:
        ctx.set_transfer(False)


EPOCH_RANGE = "power: epoch range"
NO_EPOCHS = "power before epochs_set" + STATE


def test_wtheta_epochs(full, proj_only):
    from chomp_amd import _lib
    S, A, E = _lib.ChompScopeError, ValueError, _lib.ChompError
    ctx, D, name = full.ctx, float(full.D[0]), "wtheta_epochs"
    GG, HF, EX = _lib.P_GG, _lib.P_GG | _lib.P_HALOFIT, _lib.P_GG | _lib.P_EXTRAPOLATE
    _refused(S, "wtheta_epochs: fp64 only (the narrowed precision modes belong to chomp_wtheta)",
             _with_precision, ctx, _call, ctx, name, GG, 2, D)
    _refused(S, "wtheta_epochs: HaloFit spectra are evaluated by chomp_wtheta", _call, ctx, name, HF, 2, D)
    _refused(S, "wtheta_epochs: extrapolated spectra are evaluated by chomp_wtheta", _call, ctx, name, EX, 2, D)
    _refused(S, "wtheta_epochs: the wiggle transfer function is evaluated by chomp_wtheta",
             _with_wiggle, proj_only, _call, proj_only, name, GG, 2, D)
    _refused(E, "wtheta_epochs before kernel_setup" + STATE, _call, _bare(), name, GG, 2, D)
    _refused(A, "wtheta_epochs: n * n_epoch too large", _too_large, ctx, name, D)
    _refused(A, "wtheta_epochs: k range / D_z", _call, ctx, name, GG, 2, D, BAD_K)
    _refused(A, "wtheta_epochs: k range / D_z", _call, ctx, name, GG, 2, 0.0)
    _refused(A, EPOCH_RANGE, _call, ctx, name, GG, 2, D, K, 1)
    # precedence: the scope before the k range, the state before the scope
    _refused(S, "wtheta_epochs: HaloFit spectra are evaluated by chomp_wtheta", _call, ctx, name, HF, 2, D, BAD_K)
    _refused(E, "wtheta_epochs before kernel_setup" + STATE, _call, _bare(), name, HF, 2, D)
    assert _call(ctx, name, GG, 2, D).shape == (2, 3)


def test_wtheta_sets(full, proj_only, wiggle_sets):
    from chomp_amd import _lib
    S, A, E = _lib.ChompScopeError, ValueError, _lib.ChompError
    ctx, D, name = full.ctx, numpy.array(full.D), "wtheta_sets"
    GG, HF, EX = _lib.P_GG, _lib.P_GG | _lib.P_HALOFIT, _lib.P_GG | _lib.P_EXTRAPOLATE
    before = "wtheta_sets before kernel_setup_sets / kernel_setup_pairs" + STATE
    count = "wtheta_sets: n_epoch is not the number of sets of the last kernel_setup_sets / kernel_setup_pairs"
    _refused(S, "wtheta_sets: fp64 only (the narrowed precision modes belong to chomp_wtheta)",
             _with_precision, ctx, _call, ctx, name, GG, 2, D)
    _refused(S, "wtheta_sets: HaloFit spectra are evaluated by chomp_wtheta", _call, ctx, name, HF, 2, D)
    _refused(S, "wtheta_sets: extrapolated spectra are evaluated by chomp_wtheta", _call, ctx, name, EX, 2, D)
    _refused(S, "wtheta_sets: the wiggle transfer function is evaluated by chomp_wtheta",
             _call, wiggle_sets, name, GG, 2, D)
    _refused(E, before, _call, proj_only, name, GG, 2, D)
    _refused(A, count, _call, ctx, name, GG, 3, numpy.ones(3))
    _refused(A, "wtheta_sets: n * n_epoch too large", _too_large, ctx, name, D)
    _refused(A, "wtheta_sets: k range", _call, ctx, name, GG, 2, D, BAD_K)
    _refused(A, "wtheta_sets: D_z", _call, ctx, name, GG, 2, numpy.array([1.0, 0.0]))
    _refused(A, EPOCH_RANGE, _call, ctx, name, GG, 2, D, K, 1)
    # precedence: the scope before the k range, the state before the scope, the row count before D_z
    _refused(S, "wtheta_sets: HaloFit spectra are evaluated by chomp_wtheta", _call, ctx, name, HF, 2, D, BAD_K)
    _refused(E, before, _call, proj_only, name, HF, 2, D)
    _refused(A, count, _call, ctx, name, GG, 3, numpy.array([0.0, 1.0, 1.0]))
    assert _call(ctx, name, GG, 2, D).shape == (2, 3)


def test_xi3d_epochs(full):
    """No projection set-up is needed: the state refused is check_power's, after the scope."""
    from chomp_amd import _lib, defaults
    S, A, E = _lib.ChompScopeError, ValueError, _lib.ChompError
    ctx, name = full.ctx, "xi3d_epochs"
    GG, HF, EX = _lib.P_GG, _lib.P_GG | _lib.P_HALOFIT, _lib.P_GG | _lib.P_EXTRAPOLATE
    _refused(S, "xi3d_epochs: fp64 only (the narrowed precision modes belong to chomp_xi3d)",
             _with_precision, ctx, _call, ctx, name, GG, 2, None)
    _refused(S, "xi3d_epochs: HaloFit spectra are evaluated by chomp_xi3d", _call, ctx, name, HF, 2, None)
    _refused(S, "xi3d_epochs: extrapolated spectra are evaluated by chomp_xi3d", _call, ctx, name, EX, 2, None)
    bare = _bare()
    _refused(S, "xi3d_epochs: the wiggle transfer function is evaluated by chomp_xi3d",
             _with_wiggle, bare, _call, bare, name, GG, 2, None)
    saved = copy.deepcopy(defaults.default_precision)
    try:
        defaults.default_precision.update(divmax=22)
        deep = _bare()
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)
    assert deep.config.divmax == 22
    _refused(S, "xi3d_epochs: divmax beyond the node table (level 20) is evaluated by chomp_xi3d",
             _call, deep, name, GG, 2, None)
    _refused(E, NO_EPOCHS, _call, bare, name, GG, 2, None)
    _refused(A, "xi3d_epochs: n * n_epoch too large", _too_large, ctx, name, None)
    _refused(A, "xi3d_epochs: k range", _call, ctx, name, GG, 2, None, BAD_K)
    _refused(A, EPOCH_RANGE, _call, ctx, name, GG, 2, None, K, 1)
    # precedence: the scope before the k range and before the epochs
    _refused(S, "xi3d_epochs: HaloFit spectra are evaluated by chomp_xi3d", _call, ctx, name, HF, 2, None, BAD_K)
    _refused(S, "xi3d_epochs: HaloFit spectra are evaluated by chomp_xi3d", _call, bare, name, HF, 2, None)
    assert _call(ctx, name, GG, 2, None).shape == (2, 3)


def test_cell_epochs(full, proj_only):
    from chomp_amd import _lib
    S, A, E = _lib.ChompScopeError, ValueError, _lib.ChompError
    ctx, D, name = full.ctx, float(full.D[0]), "cell_epochs"
    GG, HF, EX = _lib.P_GG, _lib.P_GG | _lib.P_HALOFIT, _lib.P_GG | _lib.P_EXTRAPOLATE
    _refused(S, "cell_epochs: fp64 only (no narrowed precision mode evaluates C_l)",
             _with_precision, ctx, _call, ctx, name, GG, 2, D)
    _refused(S, "cell_epochs: HaloFit spectra are evaluated by chomp_cell", _call, ctx, name, HF, 2, D)
    _refused(S, "cell_epochs: extrapolated spectra are evaluated by chomp_cell", _call, ctx, name, EX, 2, D)
    _refused(S, "cell_epochs: the wiggle transfer function is evaluated by chomp_cell",
             _with_wiggle, proj_only, _call, proj_only, name, GG, 2, D)
    _refused(E, "cell_epochs before kernel_setup" + STATE, _call, _bare(), name, GG, 2, D)
    _refused(A, "cell_epochs: n * n_epoch too large", _too_large, ctx, name, D)
    _refused(A, "cell_epochs: D_z", _call, ctx, name, GG, 2, 0.0)
    _refused(A, EPOCH_RANGE, _call, ctx, name, GG, 2, D, K, 1)
    # precedence: the scope before D_z, the state before the scope
    _refused(S, "cell_epochs: HaloFit spectra are evaluated by chomp_cell", _call, ctx, name, HF, 2, 0.0)
    _refused(E, "cell_epochs before kernel_setup" + STATE, _call, _bare(), name, HF, 2, D)
    assert _call(ctx, name, GG, 2, D).shape == (2, 3)


def test_cell_sets(full, proj_only, wiggle_sets):
    from chomp_amd import _lib
    S, A, E = _lib.ChompScopeError, ValueError, _lib.ChompError
    ctx, D, name = full.ctx, numpy.array(full.D), "cell_sets"
    GG, HF, EX = _lib.P_GG, _lib.P_GG | _lib.P_HALOFIT, _lib.P_GG | _lib.P_EXTRAPOLATE
    before = "cell_sets before kernel_setup_sets / kernel_setup_pairs" + STATE
    count = "cell_sets: n_epoch is not the number of sets of the last kernel_setup_sets / kernel_setup_pairs"
    _refused(S, "cell_sets: fp64 only (no narrowed precision mode evaluates C_l)",
             _with_precision, ctx, _call, ctx, name, GG, 2, D)
    _refused(S, "cell_sets: HaloFit spectra are evaluated by chomp_cell", _call, ctx, name, HF, 2, D)
    _refused(S, "cell_sets: extrapolated spectra are evaluated by chomp_cell", _call, ctx, name, EX, 2, D)
    _refused(S, "cell_sets: the wiggle transfer function is evaluated by chomp_cell",
             _call, wiggle_sets, name, GG, 2, D)
    _refused(E, before, _call, proj_only, name, GG, 2, D)
    _refused(A, count, _call, ctx, name, GG, 3, numpy.ones(3))
    _refused(A, "cell_sets: n * n_epoch too large", _too_large, ctx, name, D)
    _refused(A, "cell_sets: D_z", _call, ctx, name, GG, 2, numpy.array([1.0, 0.0]))
    _refused(A, EPOCH_RANGE, _call, ctx, name, GG, 2, D, K, 1)
    # precedence: the scope before D_z, the state before the scope, the row count before D_z
    _refused(S, "cell_sets: HaloFit spectra are evaluated by chomp_cell", _call, ctx, name, HF, 2,
             numpy.array([0.0, 1.0]))
    _refused(E, before, _call, proj_only, name, HF, 2, D)
    _refused(A, count, _call, ctx, name, GG, 3, numpy.array([0.0, 1.0, 1.0]))
    assert _call(ctx, name, GG, 2, D).shape == (2, 3)
