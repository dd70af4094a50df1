"""What the covariance C calls refuse -- chomp_covariance_table through chomp_covariance_ng, the
block-axis and the CovarianceFourier calls included -- by exception class and FULL message, and
which refusal comes first when two apply.  The texts are literals, one table per entry point: the
calls share their refusals' code, and a shared message that named the wrong call would still hold
the substrings the other tests match.

Every case returns before a kernel: nothing is launched beyond the fixtures' set-ups and the valid
call before and after each table, whose results are equal bit for bit (a refusal leaves nothing
behind).  The staged context holds two correlations (three blocks: two diagonal, one cross) and the
calls take three pairs of angles.

The "npoints too large" refusals of the dynamic LDS are pinned on contexts of the largest
projection set-up (cosmo_npoints 240, window_npoints 360: kernel_setup refuses more), where the
two windows of a set-up take 9 * 240 - 8 + 8 * 359 = 5024 doubles (40 kB) and fit, and the four
of a cross block 7896 doubles (63 kB) before anything else: test_lds_refusals.  Not pinned, because
arithmetic shows that no context reaches them:
    kernel_ng_setup: cosmo/window_npoints too large for the four windows of a cross block -- it
        needs a kernel_ssc_setup_cross that passed, whose kernel has the same static LDS (2848 B)
        and 5 n_sigma - 4 doubles MORE of dynamic LDS for the same windows;
    covariance_ssc_cross / covariance_ssc_blocks: halo/kernel_npoints too large for the two
        responses of a cross block -- 24 (halo_npoints - 1) + 5 kernel_npoints - 4 doubles; a
        context takes halo_npoints <= 256 and the calls kernel_npoints <= 256, so at most 7396
        doubles (59168 B) beside 2272 / 3680 B of static LDS: under 64 kB;
and because no sequence of calls reaches them (the checks guard states the calls before them
already refuse): "the snapshots are of another configuration" (covariance_cross_stage takes
snapshots of this configuration alone), the slot checks of calls that come after a set-up from the
slots (staging a slot again drops that set-up), and covariance_cross_stage's "both contexts must
be on one device" on a machine with one device."""
import copy
import ctypes

import numpy
import pytest

from test_gpu_covariance_blocks import setup_single, three_correlations
from test_gpu_covariance_cross import D2R
from test_gpu_covariance_ssc_blocks import multi

pytestmark = pytest.mark.gpu
STATE = " (code -3)"                         # (how _lib words CHOMP_ERR_STATE)
EPOCH_RANGE = "power: epoch range"
NO_EPOCHS = "power before epochs_set"
SETS = " before kernel_setup_pairs / kernel_setup_sets" + STATE
COUNT = ": n_corr is not the number of sets of the last kernel_setup_pairs / kernel_setup_sets" + STATE
ORDER = (": the sets are of Bessel order 2 (the covariance of w(theta) takes the windows of a "
         "Kernel, order 0)" + STATE)
MANY = ": more than 65535 blocks (a grid's z dimension)"
SLOTS = " before covariance_cross_stage of both slots" + STATE
APART = ": the four windows have no redshift in common (kernel.py:910-916 would give z_min >= z_max)"
N_MANY = 362                                 # 362 * 363 / 2 = 65703 blocks


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def raw(ctx, name, *args):
    """The C entry point itself (the Python layer sizes and allocates before it calls)."""
    ctx._check(getattr(ctx._L, "chomp_" + name)(ctx._h, *args))


def _refused(cls, text, fn, *args, **kws):
    with pytest.raises(cls) as info:
        fn(*args, **kws)
    assert type(info.value) is cls and str(info.value) == text, (str(info.value), text)


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return numpy.array_equal(numpy.asarray(a), numpy.asarray(b), equal_nan=True)


def _with_precision(make, **precision):
    """make() under other default_precision values (a context snapshots them when it is made)."""
    from chomp_amd import defaults
    saved = copy.deepcopy(defaults.default_precision)
    try:
        defaults.default_precision.update(precision)
        return make()
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)


def _bare(**precision):
    """A fresh context: neither epochs nor a projection set-up (nothing is launched)."""
    from chomp_amd import cosmology
    return _with_precision(cosmology._context, **precision)


class Full(object):
    """Two correlations on one context: their kernels as projection sets, two epochs of a
    HaloGrid at their z_bar with the families of the super-sample response, every block's
    sigma^2 knots, and what the single-block calls take."""

    def __init__(self):
        from chomp_amd import _lib, correlation, covariance, grid, kernel
        self.corrs = three_correlations()[:2]
        self.kernels = [c.kernel for c in self.corrs]
        first = multi(self.corrs).covariance_list[0][0]
        kc = first.kernel
        self.area, self.j0 = first.area, first._j0_limit
        self.kt = (kc.ln_ktheta_min, kc.ln_ktheta_max, kc._j0_ssc_limit)
        c = numpy.array([b.center for b in first.annular_bins])
        self.ta, self.tb = c[[0, 0, 1]], c[[0, 1, 2]]
        self.pairs = numpy.concatenate([self.ta, self.tb])
        self.neg = numpy.concatenate([self.ta, -self.tb])
        self.poisson = 1e-9 * (1.0 + numpy.arange(12.0).reshape(3, 4))
        self.hg = grid.HaloGrid(numpy.zeros(2))
        self.ctx = self.hg.ctx
        self.code = correlation._POWER["power_mm"][0]
        kernel.Kernel._setup_pairs_on(self.ctx, self.kernels)
        info = self.ctx.kernel_info_sets()
        self.z_bar, self.D = info["z_bar"], info["D_zbar"]
        self.hg.set_parameters(z=self.z_bar)
        self.hg.setup("power_mm", families=_lib.FAM_SSC)
        self.ranges = self.ctx.covariance_ssc_blocks_range(2)
        self.ln_chi, self.sigma2 = covariance.CovarianceMulti._ssc_blocks_knots(
            [k.cosmo for k in self.kernels], self.ranges)
        self.ep = numpy.array([0, 1], dtype=numpy.uintp)
        self.out = numpy.empty(16)

    def single(self):
        setup_single(self.ctx, self.kernels[0])

    def stage(self, which=None):
        """Both slots: correlation 0 and correlation 1 (ends with kernel 1's kernel_setup)."""
        ctx, which = self.ctx, self.code if which is None else which
        setup_single(ctx, self.kernels[0])
        ctx.covariance_cross_stage(0, ctx, which, 0)
        setup_single(ctx, self.kernels[1])
        ctx.covariance_cross_stage(1, ctx, which, 1)

    def ssc_setup(self, cross=False, with_table=True, b=0):
        return self.ctx.kernel_ssc_setup(self.kt[0], self.kt[1], self.kt[2], self.ln_chi[b],
                                         self.sigma2[b], with_table=with_table, cross=cross)

    def ssc_blocks(self, ep=(0, 1), kt=None, ln_chi=None, sigma2=None, area=None, ta=None, tb=None):
        kt = self.kt if kt is None else kt
        return self.ctx.covariance_ssc_blocks(
            ep, kt[0], kt[1], kt[2], self.ln_chi if ln_chi is None else ln_chi,
            self.sigma2 if sigma2 is None else sigma2, self.area if area is None else area,
            self.ta if ta is None else ta, self.tb if tb is None else tb)

    def blocks(self, ep=(0, 1), j0=None, area=None, poisson=None, ta=None, tb=None, which=None):
        return self.ctx.covariance_blocks(
            self.code if which is None else which, ep, self.j0 if j0 is None else j0,
            self.area if area is None else area, self.poisson if poisson is None else poisson,
            self.ta if ta is None else ta, self.tb if tb is None else tb)

    def epp(self):
        return self.ep.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))


@pytest.fixture(scope="module")
def full():
    import torch
    assert torch.cuda.is_available()
    return Full()


@pytest.fixture(scope="module")
def proj_only(full):
    """kernel_setup only: no sets, no epochs, no covariance state."""
    from chomp_amd import cosmology
    ctx = cosmology._context()
    setup_single(ctx, full.kernels[0])
    return ctx


@pytest.fixture(scope="module")
def sets_only(full):
    """The two projection sets and a kernel_setup, no epochs."""
    from chomp_amd import cosmology, kernel
    ctx = cosmology._context()
    kernel.Kernel._setup_pairs_on(ctx, full.kernels)
    setup_single(ctx, full.kernels[0])
    return ctx


@pytest.fixture(scope="module")
def order2(full):
    """Two projection sets of Bessel order 2, no epochs."""
    from chomp_amd import cosmology, kernel
    ctx = cosmology._context()
    lens = [kernel.GalaxyGalaxyLensingKernel(k._ktheta[0], k._ktheta[1], k.window_function_a,
                                             k.window_function_b, k.cosmo) for k in full.kernels]
    kernel.Kernel._setup_pairs_on(ctx, lens)
    return ctx


@pytest.fixture(scope="module")
def many(full):
    """N_MANY projection sets (one kernel, again and again): more than 65535 blocks."""
    from chomp_amd import cosmology, kernel
    ctx = cosmology._context()
    kernel.Kernel._setup_pairs_on(ctx, [full.kernels[0]] * N_MANY)
    return ctx


@pytest.fixture(scope="module")
def apart():
    """Two windows with no redshift in common: as the two projection sets, and as the two slots
    of a cross block (windows only), on a context whose kernel_setup is the second's."""
    from chomp_amd import _lib, cosmology, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    lo = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 0.5, 0.3, 0.1), cm)
    hi = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
    kernels = [kernel.Kernel(1e-6 * D2R, 100.0 * D2R, w, w, cm) for w in (lo, hi)]
    ctx = cosmology._context()
    kernel.Kernel._setup_pairs_on(ctx, kernels)
    for slot, k in enumerate(kernels):
        setup_single(ctx, k)
        ctx.covariance_cross_stage(slot, ctx, _lib.CROSS_WINDOWS)
    return ctx


class Big(object):
    """The two correlations of `full` on a context of the largest projection set-up: two epochs
    with the families of the super-sample response, the two projection sets, and both slots of
    the cross block staged with their spectra (ends with kernel 1's kernel_setup)."""

    def __init__(self, F, **precision):
        from chomp_amd import _lib, grid, kernel
        self.hg = _with_precision(lambda: grid.HaloGrid(numpy.zeros(2)), cosmo_npoints=240,
                                  window_npoints=360, **precision)
        ctx = self.ctx = self.hg.ctx
        assert ctx.config.cosmo_npoints == 240 and ctx.config.window_npoints == 360
        kernel.Kernel._setup_pairs_on(ctx, F.kernels)
        self.hg.set_parameters(z=F.z_bar)
        self.hg.setup("power_mm", families=_lib.FAM_SSC)
        for slot, k in enumerate(F.kernels):
            setup_single(ctx, k)
            ctx.covariance_cross_stage(slot, ctx, F.code, slot)


@pytest.fixture(scope="module")
def big(full):
    return Big(full)


def _lib_names():
    from chomp_amd import _lib
    return _lib, _lib.ChompScopeError, ValueError, _lib.ChompError


def test_null_context():
    """Every covariance call returns CHOMP_ERR_ARG for a null context (there is no message); so
    does chomp_covariance_ng_blocks_plan, which takes no context, for its all-zero arguments."""
    _lib = _lib_names()[0]
    L = _lib.lib()
    names = [n for n in _lib.EXPORTS if n.startswith(("chomp_covariance_", "chomp_kernel_ssc_",
                                                      "chomp_kernel_ng_"))]
    assert len(names) == 27, names
    for name in names:
        fn = getattr(L, name)
        args = [0.0 if t is ctypes.c_double else 0 if t in (ctypes.c_int, ctypes.c_size_t) else None
                for t in fn.argtypes]
        assert fn(*args) == _lib.ERR_ARG, name


def test_covariance_table(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_table"
    F.single()
    D, n = float(F.D[0]), ctx.config.kernel_npoints
    o = numpy.empty(n)
    before = ctx.covariance_table(F.code, 0, D)
    _refused(E, "covariance_table before kernel_setup" + STATE, _bare().covariance_table, F.code, 0, D)
    _refused(E, NO_EPOCHS + STATE, proj_only.covariance_table, F.code, 0, D)
    _refused(A, EPOCH_RANGE, ctx.covariance_table, F.code, 2, D)
    _refused(A, "covariance_table: D_z", ctx.covariance_table, F.code, 0, 0.0)
    _refused(A, "covariance_table: length must be kernel_npoints", raw, ctx, name, F.code, 0, D,
             P(o), None, None, n - 1)
    # precedence: the state before D_z, check_power before D_z, D_z before the length
    _refused(E, "covariance_table before kernel_setup" + STATE, _bare().covariance_table, F.code, 0, 0.0)
    _refused(A, EPOCH_RANGE, ctx.covariance_table, F.code, 2, 0.0)
    _refused(A, "covariance_table: D_z", raw, ctx, name, F.code, 0, 0.0, P(o), None, None, n - 1)
    assert _same(ctx.covariance_table(F.code, 0, D), before)


def _gaussian_table(F, name, what, call, pre, no_table):
    """covariance_gaussian and covariance_gaussian_cross: `pre` the scalars after area."""
    _lib, S, A, E = _lib_names()
    ctx = F.ctx
    before = call(F.j0, F.area, F.ta, F.tb)

    def c(ctx_, j0, area, th, n=3, mem=_lib.HOST):
        raw(ctx_, name, j0, area, *pre, P(th), n, P(F.out), mem)
    _refused(A, name + ": bad args", c, ctx, F.j0, F.area, F.pairs, 0)
    _refused(A, name + ": bad args", c, ctx, F.j0, F.area, None)
    _refused(A, name + ": mem", c, ctx, F.j0, F.area, F.pairs, 3, 7)
    _refused(E, name + " before " + what + STATE, c, no_table, F.j0, F.area, F.pairs)
    _refused(A, name + ": j0_limit and area must be positive", c, ctx, 0.0, F.area, F.pairs)
    _refused(A, name + ": j0_limit and area must be positive", c, ctx, F.j0, 0.0, F.pairs)
    _refused(A, name + ": theta must be positive", c, ctx, F.j0, F.area, F.neg)
    # precedence: the arguments before mem, mem before the state, the state before the area, the
    # area before theta
    _refused(A, name + ": bad args", c, ctx, F.j0, F.area, F.pairs, 0, 7)
    _refused(A, name + ": mem", c, no_table, F.j0, F.area, F.pairs, 3, 7)
    _refused(E, name + " before " + what + STATE, c, no_table, F.j0, 0.0, F.pairs)
    _refused(A, name + ": j0_limit and area must be positive", c, ctx, F.j0, 0.0, F.neg)
    assert _same(call(F.j0, F.area, F.ta, F.tb), before)


def test_covariance_gaussian(full, proj_only):
    F, ctx = full, full.ctx
    F.single()
    ctx.covariance_table(F.code, 0, float(F.D[0]))
    _gaussian_table(F, "covariance_gaussian", "covariance_table",
                    lambda j0, area, ta, tb: ctx.covariance_gaussian(j0, area, 1e-9, 2e-9, ta, tb),
                    (1e-9, 2e-9), proj_only)


def test_covariance_cross_stage(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_cross_stage"
    F.stage()
    D = (float(F.D[0]), float(F.D[1]))
    before = ctx.covariance_table_cross(*D)
    wiggle = _bare()
    wiggle.set_transfer(True)
    setup_single(wiggle, F.kernels[0])
    bare = _bare()
    _refused(A, name + ": bad args", raw, ctx, name, 0, None, F.code, 0)
    _refused(A, name + ": slot must be 0 or 1", ctx.covariance_cross_stage, 2, ctx, F.code, 0)
    _refused(A, name + ": slot must be 0 or 1", ctx.covariance_cross_stage, -1, ctx, F.code, 0)
    _refused(E, name + ": the source context has no kernel_setup" + STATE,
             ctx.covariance_cross_stage, 0, bare, F.code, 0)
    _refused(E, name + ": source: " + NO_EPOCHS + STATE, ctx.covariance_cross_stage, 0, proj_only, F.code, 0)
    _refused(A, name + ": source: " + EPOCH_RANGE, ctx.covariance_cross_stage, 0, ctx, F.code, 2)
    _refused(S, name + ": both contexts must share one configuration and transfer function",
             ctx.covariance_cross_stage, 0, wiggle, _lib.CROSS_WINDOWS)
    # precedence: the slot before the source's state, the source's spectrum before the scope
    _refused(A, name + ": slot must be 0 or 1", ctx.covariance_cross_stage, 2, bare, F.code, 0)
    _refused(E, name + ": source: " + NO_EPOCHS + STATE, ctx.covariance_cross_stage, 0, wiggle, F.code, 0)
    # (no refusal unstaged a slot)
    assert _same(ctx.covariance_table_cross(*D), before)
    F.stage()
    assert _same(ctx.covariance_table_cross(*D), before)


def test_covariance_table_cross(full, proj_only, apart):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_table_cross"
    F.stage()
    D, n = (float(F.D[0]), float(F.D[1])), ctx.config.kernel_npoints
    o = numpy.empty(n)
    before = ctx.covariance_table_cross(*D)
    windows = name + ": a slot holds windows only (CHOMP_CROSS_WINDOWS)" + STATE
    _refused(E, name + SLOTS, proj_only.covariance_table_cross, *D)
    _refused(E, windows, apart.covariance_table_cross, *D)
    _refused(A, name + ": D_a, D_b", ctx.covariance_table_cross, 0.0, D[1])
    _refused(A, name + ": D_a, D_b", ctx.covariance_table_cross, D[0], 0.0)
    _refused(A, name + ": length must be kernel_npoints", raw, ctx, name, D[0], D[1], P(o), None,
             None, n + 1)
    # precedence: the slots before D, windows only before D, D before the length
    _refused(E, name + SLOTS, proj_only.covariance_table_cross, 0.0, D[1])
    _refused(E, windows, apart.covariance_table_cross, 0.0, D[1])
    _refused(A, name + ": D_a, D_b", raw, ctx, name, 0.0, D[1], P(o), None, None, n + 1)
    assert _same(ctx.covariance_table_cross(*D), before)


def test_covariance_gaussian_cross(full, proj_only):
    F, ctx = full, full.ctx
    F.stage()
    ctx.covariance_table_cross(float(F.D[0]), float(F.D[1]))
    p = tuple(float(v) for v in F.poisson[1])
    _gaussian_table(F, "covariance_gaussian_cross", "covariance_table_cross",
                    lambda j0, area, ta, tb: ctx.covariance_gaussian_cross(j0, area, p, ta, tb),
                    p, proj_only)


def _sets_table(name, call, F, proj_only, sets_only, order2, many, after_sets=()):
    """What chomp_covariance_blocks, chomp_covariance_ssc_blocks and _ssc_blocks_range ask of
    the sets; call(ctx, n_corr, bad_epoch)."""
    _lib, S, A, E = _lib_names()
    _refused(E, name + SETS, call, proj_only, 2, False)
    _refused(E, name + COUNT, call, F.ctx, 1, False)
    _refused(E, name + COUNT, call, F.ctx, 3, False)
    _refused(E, name + ORDER, call, order2, 2, False)
    _refused(A, name + MANY, call, many, N_MANY, False)
    # precedence: n_corr before the Bessel order, the sets before check_power
    _refused(E, name + COUNT, call, order2, 3, False)
    _refused(E, name + COUNT, call, F.ctx, 3, True)
    _refused(E, name + ORDER, call, order2, 2, True)
    _refused(E, name + COUNT, call, sets_only, 3, False)


def test_covariance_blocks(full, proj_only, sets_only, order2, many):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_blocks"
    before = F.blocks()
    tables = [ctx.covariance_blocks_table(b) for b in range(3)]

    def c(ctx_, n_corr=2, ep=True, j0=F.j0, area=F.area, po=F.poisson, th=F.pairs, n=3,
          mem=_lib.HOST, which=F.code):
        raw(ctx_, name, which, n_corr, F.epp() if ep else None, j0, area, P(po), P(th), n, P(F.out), mem)

    def sets(ctx_, n_corr, bad_epoch):
        ep = numpy.full(n_corr, 5 if bad_epoch else 0, dtype=numpy.uintp)
        raw(ctx_, name, F.code, n_corr, ep.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), F.j0,
            F.area, P(numpy.zeros(2 * n_corr * (n_corr + 1))), P(F.pairs), 3, P(F.out), _lib.HOST)
    _refused(A, name + ": bad args", c, ctx, 0)
    _refused(A, name + ": bad args", c, ctx, n=0)
    _refused(A, name + ": bad args", c, ctx, ep=False)
    _refused(A, name + ": bad args", c, ctx, po=None)
    _refused(A, name + ": mem", c, ctx, mem=7)
    _sets_table(name, sets, F, proj_only, sets_only, order2, many)
    _refused(A, name + ": n_pairs * n_blocks too large", c, ctx, n=1 << 30)
    _refused(A, name + ": correlation 1: " + EPOCH_RANGE, F.blocks, (0, 2))
    _refused(E, name + ": correlation 0: " + NO_EPOCHS + STATE, c, sets_only)
    _refused(A, name + ": j0_limit and area must be positive", F.blocks, j0=0.0)
    _refused(A, name + ": j0_limit and area must be positive", F.blocks, area=0.0)
    _refused(A, name + ": theta must be positive", F.blocks, tb=-F.tb)
    # precedence: mem before the sets, the product before check_power, check_power before the
    # area, the area before theta
    _refused(A, name + ": mem", c, proj_only, mem=7)
    F.ep[1] = 5
    try:
        _refused(A, name + ": n_pairs * n_blocks too large", c, ctx, n=1 << 30)
        _refused(A, name + ": correlation 1: " + EPOCH_RANGE, c, ctx, area=0.0)
    finally:
        F.ep[1] = 1
    _refused(A, name + ": j0_limit and area must be positive", c, ctx, area=0.0, th=F.neg)
    assert _same(F.blocks(), before)
    assert _same([ctx.covariance_blocks_table(b) for b in range(3)], tables)


def test_covariance_blocks_table(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_blocks_table"
    F.blocks()
    n = ctx.config.kernel_npoints
    o = numpy.empty(n)
    before = [ctx.covariance_blocks_table(b) for b in range(3)]
    assert not numpy.any(before[0][1][1:]) and numpy.any(before[1][1][1:])
    _refused(E, name + " before covariance_blocks" + STATE, proj_only.covariance_blocks_table, 0)
    _refused(A, name + ": block", ctx.covariance_blocks_table, 3)
    _refused(A, name + ": length must be kernel_npoints", raw, ctx, name, 0, P(o), None, None, None, n - 1)
    # precedence: the state before the block, the block before the length
    _refused(E, name + " before covariance_blocks" + STATE, proj_only.covariance_blocks_table, 3)
    _refused(A, name + ": block", raw, ctx, name, 3, P(o), None, None, None, n - 1)
    assert _same([ctx.covariance_blocks_table(b) for b in range(3)], before)


def _fourier_ready(F):
    """Both slots, the z_bar of the four pairs and the four tables; (info, tables)."""
    ctx = F.ctx
    F.stage()
    info = ctx.covariance_fourier_zbar(numpy.linspace(0.0, 2.0, 64))
    ln_l = numpy.linspace(numpy.log(10.0), numpy.log(1e4), ctx.config.corr_npoints)
    return info, ln_l, ctx.covariance_fourier_table(F.code, [0, 1, 0, 1], ln_l)


def test_covariance_fourier_zbar(full, proj_only, apart):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_fourier_zbar"
    z = numpy.linspace(0.0, 2.0, 64)
    info = numpy.empty(28)
    before = _fourier_ready(F)[0]
    _refused(A, name + ": bad args", raw, ctx, name, None, 64, P(info))
    _refused(A, name + ": the z grid must hold 1..256 points", raw, ctx, name, P(z), 0, P(info))
    _refused(A, name + ": the z grid must hold 1..256 points", ctx.covariance_fourier_zbar,
             numpy.linspace(0.0, 2.0, 257))
    _refused(A, name + ": corr_npoints must be at least 4", _bare(corr_npoints=3).covariance_fourier_zbar, z)
    _refused(E, name + SLOTS, proj_only.covariance_fourier_zbar, z)
    _refused(S, name + ": the windows of pair a1b2 have no redshift in common",
             apart.covariance_fourier_zbar, z)
    # precedence: the grid before the slots
    _refused(A, name + ": the z grid must hold 1..256 points", raw, proj_only, name, P(z), 0, P(info))
    assert _same(ctx.covariance_fourier_zbar(z), before)


def test_covariance_fourier_table(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_fourier_table"
    _, ln_l, before = _fourier_ready(F)
    scope = (name + ": the tables are built from Halo.power_mm (CHOMP_P_MM, with or without "
             "CHOMP_P_EXTRAPOLATE)")
    ep = (ctypes.c_size_t * 4)(0, 1, 0, 1)
    _refused(A, name + ": bad args", raw, ctx, name, F.code, ep, None, ln_l.size, None, None, None)
    _refused(A, name + ": bad args", raw, ctx, name, F.code, None, P(ln_l), ln_l.size, None, None, None)
    _refused(E, name + " before covariance_fourier_zbar" + STATE, proj_only.covariance_fourier_table,
             F.code, [0, 1, 0, 1], ln_l)
    _refused(S, scope, ctx.covariance_fourier_table, _lib.P_GG, [0, 1, 0, 1], ln_l)
    _refused(S, scope, ctx.covariance_fourier_table, F.code | _lib.P_HALOFIT, [0, 1, 0, 1], ln_l)
    _refused(A, EPOCH_RANGE, ctx.covariance_fourier_table, F.code, [0, 1, 0, 2], ln_l)
    _refused(A, name + ": length must be corr_npoints", ctx.covariance_fourier_table, F.code,
             [0, 1, 0, 1], ln_l[:-1])
    _refused(A, name + ": ln l knots must increase", ctx.covariance_fourier_table, F.code,
             [0, 1, 0, 1], ln_l[::-1])
    # precedence: the state before the scope, the scope before check_power, check_power before
    # the length, the length before the knots
    _refused(E, name + " before covariance_fourier_zbar" + STATE, proj_only.covariance_fourier_table,
             _lib.P_GG, [0, 1, 0, 1], ln_l)
    _refused(S, scope, ctx.covariance_fourier_table, _lib.P_GG, [0, 1, 0, 2], ln_l)
    _refused(A, EPOCH_RANGE, ctx.covariance_fourier_table, F.code, [0, 1, 0, 2], ln_l[:-1])
    _refused(A, name + ": length must be corr_npoints", ctx.covariance_fourier_table, F.code,
             [0, 1, 0, 1], ln_l[::-1][:-1])
    assert _same(ctx.covariance_fourier_table(F.code, [0, 1, 0, 1], ln_l), before)


def test_covariance_fourier_gaussian(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_fourier_gaussian"
    _fourier_ready(F)
    l = numpy.array([20.0, 200.0, 2000.0])
    x = numpy.concatenate([numpy.log(l), l])
    before = ctx.covariance_fourier_gaussian(x)

    def c(ctx_, x_=x, n=3, mem=_lib.HOST):
        raw(ctx_, name, P(x_), n, P(F.out), mem)
    _refused(A, name + ": bad args", c, ctx, None)
    _refused(A, name + ": bad args", c, ctx, n=0)
    _refused(A, name + ": mem", c, ctx, mem=7)
    _refused(E, name + " before covariance_fourier_table" + STATE, c, proj_only)
    # precedence: the arguments before mem, mem before the state
    _refused(A, name + ": bad args", c, proj_only, n=0, mem=7)
    _refused(A, name + ": mem", c, proj_only, mem=7)
    assert _same(ctx.covariance_fourier_gaussian(x), before)


@pytest.mark.parametrize("cross", [False, True])
def test_kernel_ssc_setup(full, proj_only, apart, cross):
    """Both entry points word the shared refusals "kernel_ssc_setup"; the slots' are the cross
    call's own."""
    _lib, S, A, E = _lib_names()
    F, ctx = full, full.ctx
    name, who = "kernel_ssc_setup", "kernel_ssc_setup_cross" if cross else "kernel_ssc_setup"
    F.stage() if cross else F.single()
    b = 1 if cross else 0
    before = F.ssc_setup(cross=cross, b=b)
    x, y, n = F.ln_chi[b], F.sigma2[b], F.ln_chi.shape[1]
    tab = numpy.empty((ctx.config.kernel_npoints,) * 2)

    def c(ctx_, kt=F.kt, x_=x, y_=y, n_=n, with_table=1, table=None):
        raw(ctx_, who, kt[0], kt[1], kt[2], P(x_), P(y_), n_, with_table, None, P(table), None)
    _refused(A, name + ": bad args", c, ctx, x_=None)
    _refused(A, name + ": bad args", c, ctx, y_=None)
    _refused(A, name + ": table / levels need with_table", c, ctx, with_table=0, table=tab)
    _refused(E, name + " before kernel_setup" + STATE, c, _bare())
    _refused(A, name + ": ln(k theta) range / J0 limit", c, ctx, (F.kt[1], F.kt[0], F.kt[2]))
    _refused(A, name + ": ln(k theta) range / J0 limit", c, ctx, (F.kt[0], F.kt[1], 0.0))
    _refused(A, name + ": corr_npoints and kernel_npoints must be 4..256", c, ctx, n_=3)
    _refused(A, name + ": corr_npoints and kernel_npoints must be 4..256", c, ctx, n_=257)
    _refused(A, name + ": ln chi knots must increase", c, ctx, x_=numpy.ascontiguousarray(x[::-1]))
    if cross:
        _refused(E, who + SLOTS, c, proj_only)
        _refused(S, who + APART, c, apart)
        # precedence: the knots before the slots
        _refused(A, name + ": ln chi knots must increase", c, proj_only, x_=numpy.ascontiguousarray(x[::-1]))
    # precedence: with_table before the state, the state before the range, the range before the
    # counts, the counts before the knots
    _refused(A, name + ": table / levels need with_table", c, _bare(), with_table=0, table=tab)
    _refused(E, name + " before kernel_setup" + STATE, c, _bare(), (F.kt[1], F.kt[0], F.kt[2]))
    _refused(A, name + ": ln(k theta) range / J0 limit", c, ctx, (F.kt[1], F.kt[0], F.kt[2]), n_=3)
    _refused(A, name + ": corr_npoints and kernel_npoints must be 4..256", c, ctx,
             x_=numpy.ascontiguousarray(x[::-1]), n_=3)
    assert _same(F.ssc_setup(cross=cross, b=b), before)


def test_covariance_cross_range(full, proj_only, apart):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_cross_range"
    F.stage()
    before = ctx.covariance_cross_range()
    assert _same(before, F.ranges[1])
    _refused(A, name + ": bad args", raw, ctx, name, None)
    _refused(E, name + " before kernel_setup" + STATE, _bare().covariance_cross_range)
    _refused(E, name + SLOTS, proj_only.covariance_cross_range)
    _refused(S, name + APART, apart.covariance_cross_range)
    # precedence: the arguments before the state
    _refused(A, name + ": bad args", raw, _bare(), name, None)
    assert _same(ctx.covariance_cross_range(), before)


def _pair_eval_table(F, name, setup, call, not_ready, finite, bound):
    """The four ln(k theta)-pair evaluators; not_ready: a context (or a thunk that leaves
    F.ctx) without what the call needs."""
    _lib, S, A, E = _lib_names()
    ctx = F.ctx
    x = numpy.array([-2.0, -1.5, -1.0, -1.0, -0.5, 0.5])
    bad = x.copy()
    bad[4] = numpy.inf
    before = call(x[:3], x[3:])
    state = name + " before " + setup + STATE

    def c(ctx_, x_=x, n=3, out=F.out):
        raw(ctx_, name, P(x_), n, P(out))
    _refused(A, name + ": bad args", c, ctx, None)
    _refused(A, name + ": bad args", c, ctx, n=0)
    _refused(A, name + ": bad args", c, ctx, out=None)
    _refused(E, state, c, not_ready)
    if bound:
        _refused(A, name + ": too many points", c, ctx, n=1 << 31)
    if finite:
        _refused(A, name + ": ln(k theta) must be finite", c, ctx, bad)
    # precedence: the arguments before the state, the state before the bound and the values, the
    # bound before the values
    _refused(A, name + ": bad args", c, not_ready, n=0)
    _refused(E, state, c, not_ready, bad, 1 << 31)
    if bound and finite:
        _refused(A, name + ": too many points", c, ctx, bad, 1 << 31)
    assert _same(call(x[:3], x[3:]), before)


def test_kernel_ssc_raw_and_eval(full, proj_only):
    F, ctx = full, full.ctx
    F.single()
    F.ssc_setup()
    _pair_eval_table(F, "kernel_ssc_raw", "kernel_ssc_setup", ctx.kernel_ssc_raw, proj_only, True, False)
    _pair_eval_table(F, "kernel_ssc_eval", "kernel_ssc_setup", ctx.kernel_ssc_eval, proj_only, False, False)
    # a set-up without the table: the raw integrals are served, the spline is not
    raw_before = ctx.kernel_ssc_raw(numpy.array([-2.0]), numpy.array([-1.0]))
    F.ssc_setup(with_table=False)
    assert _same(ctx.kernel_ssc_raw(numpy.array([-2.0]), numpy.array([-1.0])), raw_before)
    _refused(_lib_names()[3], "kernel_ssc_eval before kernel_ssc_setup" + STATE, ctx.kernel_ssc_eval,
             numpy.array([-2.0]), numpy.array([-1.0]))


def test_covariance_ssc(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_ssc"
    F.single()
    F.ssc_setup()
    before = ctx.covariance_ssc(0, F.area, F.ta, F.tb, knots=True)

    def c(ctx_, epoch=0, area=F.area, th=F.pairs, n=3, out=F.out):
        raw(ctx_, name, epoch, area, P(th), n, P(out), None, None)
    _refused(A, name + ": bad args", c, ctx, th=None)
    _refused(A, name + ": bad args", c, ctx, n=0)
    _refused(A, name + ": bad args", c, ctx, out=None)
    _refused(E, name + " before kernel_ssc_setup" + STATE, c, proj_only)
    _refused(A, name + ": area must be positive", c, ctx, area=0.0)
    _refused(A, name + ": at most 65535 pairs a call", c, ctx, n=65536)
    _refused(A, EPOCH_RANGE, c, ctx, 2)
    _refused(A, name + ": arguments must be positive", c, ctx, th=F.neg)
    # precedence: the state before the area, the area before the pairs, the pairs before
    # check_power, check_power before the angles
    _refused(E, name + " before kernel_ssc_setup" + STATE, c, proj_only, area=0.0)
    _refused(A, name + ": area must be positive", c, ctx, area=0.0, n=65536)
    _refused(A, name + ": at most 65535 pairs a call", c, ctx, 2, n=65536)
    _refused(A, EPOCH_RANGE, c, ctx, 2, th=F.neg)
    assert _same(ctx.covariance_ssc(0, F.area, F.ta, F.tb, knots=True), before)
    # the table of a cross block is the cross call's, and the other way round
    F.stage()
    F.ssc_setup(cross=True, b=1)
    _refused(E, name + ": the kernel_ssc table is a cross block's (chomp_covariance_ssc_cross serves it)"
             + STATE, c, ctx)
    _refused(E, name + ": the kernel_ssc table is a cross block's (chomp_covariance_ssc_cross serves it)"
             + STATE, c, ctx, area=0.0)


def test_covariance_ssc_cross(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_ssc_cross"
    F.stage()
    F.ssc_setup(cross=True, b=1)
    before = ctx.covariance_ssc_cross(F.area, F.ta, F.tb, knots=True)
    state = name + " before kernel_ssc_setup_cross" + STATE

    def c(ctx_, area=F.area, th=F.pairs, n=3, out=F.out):
        raw(ctx_, name, area, P(th), n, P(out), None, None)
    _refused(A, name + ": bad args", c, ctx, th=None)
    _refused(A, name + ": bad args", c, ctx, n=0)
    _refused(A, name + ": bad args", c, ctx, out=None)
    _refused(E, state, c, proj_only)
    _refused(A, name + ": area must be positive", c, ctx, area=0.0)
    _refused(A, name + ": at most 65535 pairs a call", c, ctx, n=65536)
    _refused(A, name + ": arguments must be positive", c, ctx, th=F.neg)
    # precedence: the state before the area, the area before the pairs, the pairs before the angles
    _refused(E, state, c, proj_only, area=0.0)
    _refused(A, name + ": area must be positive", c, ctx, area=0.0, n=65536)
    _refused(A, name + ": at most 65535 pairs a call", c, ctx, th=F.neg, n=65536)
    assert _same(ctx.covariance_ssc_cross(F.area, F.ta, F.tb, knots=True), before)
    # slots that hold windows only: no response; and a single block's table is not the cross call's
    response = (name + ": the staged epochs do not hold the knot tables of the super-sample response "
                "(h_m, pp_mm, i_1_2)" + STATE)
    F.stage(_lib.CROSS_WINDOWS)
    F.ssc_setup(cross=True, b=1)
    _refused(E, response, c, ctx)
    _refused(E, response, c, ctx, area=0.0)
    F.ssc_setup(b=2)                                         # (kernel 1's, which stage() ends with)
    _refused(E, state, c, ctx)
    F.stage()
    F.ssc_setup(cross=True, b=1)
    assert _same(ctx.covariance_ssc_cross(F.area, F.ta, F.tb, knots=True), before)


def test_covariance_ssc_blocks_range(full, proj_only, sets_only, order2, many, apart):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_ssc_blocks_range"
    before = ctx.covariance_ssc_blocks_range(2)
    assert _same(before, F.ranges)
    info = numpy.empty(4 * N_MANY * (N_MANY + 1) // 2)
    _refused(A, name + ": bad args", raw, ctx, name, 2, None)
    _refused(A, name + ": bad args", raw, ctx, name, 0, P(info))
    _sets_table(name, lambda ctx_, n_corr, bad: raw(ctx_, name, n_corr, P(info)), F, proj_only,
                sets_only, order2, many)
    _refused(S, name + ": block (0, 1)" + APART, apart.covariance_ssc_blocks_range, 2)
    # precedence: the arguments before the sets, n_corr before the windows
    _refused(A, name + ": bad args", raw, proj_only, name, 0, P(info))
    _refused(E, name + COUNT, raw, apart, name, 3, P(info))
    assert _same(ctx.covariance_ssc_blocks_range(2), before)


def test_covariance_ssc_blocks(full, proj_only, sets_only, order2, many, apart):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_ssc_blocks"
    before = F.ssc_blocks()
    tables = [ctx.covariance_ssc_blocks_table(b, knots=True) for b in range(3)]
    n_sigma = F.ln_chi.shape[1]
    knots = numpy.zeros(2 * n_sigma * N_MANY * (N_MANY + 1) // 2)

    def c(ctx_, n_corr=2, ep=True, kt=F.kt, x=F.ln_chi, y=F.sigma2, n_s=n_sigma, area=F.area,
          th=F.pairs, n=3, mem=_lib.HOST):
        raw(ctx_, name, n_corr, F.epp() if ep else None, kt[0], kt[1], kt[2], P(x), P(y), n_s, area,
            P(th), n, P(F.out), mem)

    def sets(ctx_, n_corr, bad_epoch):
        ep = numpy.full(n_corr, 5 if bad_epoch else 0, dtype=numpy.uintp)
        raw(ctx_, name, n_corr, ep.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), F.kt[0], F.kt[1],
            F.kt[2], P(knots), P(knots), n_sigma, F.area, P(F.pairs), 3, P(F.out), _lib.HOST)
    _refused(A, name + ": bad args", c, ctx, 0)
    _refused(A, name + ": bad args", c, ctx, n=0)
    _refused(A, name + ": bad args", c, ctx, ep=False)
    _refused(A, name + ": bad args", c, ctx, x=None)
    _refused(A, name + ": bad args", c, ctx, y=None)
    _refused(A, name + ": mem", c, ctx, mem=7)
    _sets_table(name, sets, F, proj_only, sets_only, order2, many)
    _refused(S, name + ": block (0, 1)" + APART, c, apart)
    _refused(A, name + ": correlation 1: " + EPOCH_RANGE, F.ssc_blocks, (0, 2))
    _refused(E, name + ": correlation 0: " + NO_EPOCHS + STATE, c, sets_only)
    _refused(A, name + ": ln(k theta) range / J0 limit", F.ssc_blocks, kt=(F.kt[1], F.kt[0], F.kt[2]))
    _refused(A, name + ": ln(k theta) range / J0 limit", F.ssc_blocks, kt=(F.kt[0], F.kt[1], 0.0))
    _refused(A, name + ": corr_npoints and kernel_npoints must be 4..256", c, ctx, n_s=3)
    _refused(A, name + ": corr_npoints and kernel_npoints must be 4..256", c, ctx, n_s=257)
    bad = F.ln_chi.copy()
    bad[1] = bad[1][::-1]
    _refused(A, name + ": block 1: ln chi knots must increase", F.ssc_blocks, ln_chi=bad)
    _refused(A, name + ": area must be positive", F.ssc_blocks, area=0.0)
    _refused(A, name + ": at most 65535 pairs a call", c, ctx, n=65536)
    _refused(A, name + ": theta must be positive", F.ssc_blocks, tb=-F.tb)
    # precedence: mem before the sets, check_power before the range, the range before the
    # counts, the counts before the knots, the knots before the area, the area before the pairs,
    # the pairs before theta
    _refused(A, name + ": mem", c, proj_only, mem=7)
    F.ep[1] = 5
    try:
        _refused(A, name + ": correlation 1: " + EPOCH_RANGE, c, ctx, kt=(F.kt[1], F.kt[0], F.kt[2]))
    finally:
        F.ep[1] = 1
    _refused(A, name + ": ln(k theta) range / J0 limit", c, ctx, kt=(F.kt[1], F.kt[0], F.kt[2]), n_s=3)
    _refused(A, name + ": corr_npoints and kernel_npoints must be 4..256", c, ctx, x=bad, n_s=3)
    _refused(A, name + ": block 1: ln chi knots must increase", c, ctx, x=bad, area=0.0)
    _refused(A, name + ": area must be positive", c, ctx, area=0.0, n=65536)
    _refused(A, name + ": at most 65535 pairs a call", c, ctx, th=F.neg, n=65536)
    assert _same(F.ssc_blocks(), before)
    assert _same([ctx.covariance_ssc_blocks_table(b, knots=True) for b in range(3)], tables)


def test_covariance_ssc_blocks_table(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_ssc_blocks_table"
    F.ssc_blocks()
    before = [ctx.covariance_ssc_blocks_table(b, knots=True) for b in range(3)]
    _refused(E, name + " before covariance_ssc_blocks" + STATE, proj_only.covariance_ssc_blocks_table, 0)
    _refused(A, name + ": block", ctx.covariance_ssc_blocks_table, 3)
    # precedence: the state before the block
    _refused(E, name + " before covariance_ssc_blocks" + STATE, proj_only.covariance_ssc_blocks_table, 3)
    assert _same([ctx.covariance_ssc_blocks_table(b, knots=True) for b in range(3)], before)


def test_kernel_ng_setup(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "kernel_ng_setup"
    F.single()
    F.ssc_setup(with_table=False)
    before = ctx.kernel_ng_setup(F.j0)
    tab = numpy.empty((ctx.config.kernel_npoints,) * 2)
    need = name + ": table / levels / min need with_table"
    _refused(A, need, raw, ctx, name, F.j0, 0, P(tab), None, None)
    _refused(A, need, raw, ctx, name, F.j0, 0, None, None, P(tab))
    _refused(E, name + " before kernel_ssc_setup" + STATE, proj_only.kernel_ng_setup, F.j0)
    _refused(A, name + ": J0 limit", ctx.kernel_ng_setup, 0.0)
    # precedence: with_table before the state, the state before the limit
    _refused(A, need, raw, proj_only, name, F.j0, 0, P(tab), None, None)
    _refused(E, name + " before kernel_ssc_setup" + STATE, proj_only.kernel_ng_setup, 0.0)
    assert _same(ctx.kernel_ng_setup(F.j0), before)


def test_kernel_ng_raw_and_eval(full, proj_only):
    F, ctx = full, full.ctx
    F.single()
    F.ssc_setup(with_table=False)
    ctx.kernel_ng_setup(F.j0)
    _pair_eval_table(F, "kernel_ng_raw", "kernel_ng_setup", ctx.kernel_ng_raw, proj_only, True, True)
    _pair_eval_table(F, "kernel_ng_eval", "kernel_ng_setup", ctx.kernel_ng_eval, proj_only, False, True)
    raw_before = ctx.kernel_ng_raw(numpy.array([-2.0]), numpy.array([-1.0]))
    ctx.kernel_ng_setup(F.j0, with_table=False)
    assert _same(ctx.kernel_ng_raw(numpy.array([-2.0]), numpy.array([-1.0])), raw_before)
    _refused(_lib_names()[3], "kernel_ng_eval before kernel_ng_setup" + STATE, ctx.kernel_ng_eval,
             numpy.array([-2.0]), numpy.array([-1.0]))


def test_covariance_ng(full, proj_only):
    _lib, S, A, E = _lib_names()
    F, ctx, name = full, full.ctx, "covariance_ng"
    F.single()
    F.ssc_setup(with_table=False)
    ctx.kernel_ng_setup(F.j0)
    tri = 1e-3 * (1.0 + numpy.add.outer(numpy.arange(6.0), numpy.arange(6.0)))
    k = (1e-3, 10.0)
    before = ctx.covariance_ng(F.area, tri, k[0], k[1], F.ta, F.tb, knots=True)

    def c(ctx_, area=F.area, tri_=tri, n_tri=6, k_=k, th=F.pairs, n=3, out=F.out):
        raw(ctx_, name, area, P(tri_), n_tri, k_[0], k_[1], P(th), n, P(out), None, None)
    _refused(A, name + ": bad args", c, ctx, tri_=None)
    _refused(A, name + ": bad args", c, ctx, th=None)
    _refused(A, name + ": bad args", c, ctx, n=0)
    _refused(A, name + ": bad args", c, ctx, out=None)
    _refused(E, name + " before kernel_ng_setup" + STATE, c, proj_only)
    _refused(A, name + ": area must be positive", c, ctx, area=0.0)
    _refused(A, name + ": at most 65535 pairs a call", c, ctx, n=65536)
    _refused(A, name + ": the I_0^4 table must be 4..64 knots a side", c, ctx, n_tri=3)
    _refused(A, name + ": the I_0^4 table must be 4..64 knots a side", c, ctx, n_tri=65)
    _refused(A, name + ": the I_0^4 table's k range", c, ctx, k_=(0.0, 10.0))
    _refused(A, name + ": the I_0^4 table's k range", c, ctx, k_=(10.0, 1e-3))
    _refused(A, name + ": arguments must be positive", c, ctx, th=F.neg)
    # precedence: the state before the area, the area before the pairs, the pairs before the
    # table, the table before its range, the range before the angles
    _refused(E, name + " before kernel_ng_setup" + STATE, c, proj_only, area=0.0)
    _refused(A, name + ": area must be positive", c, ctx, area=0.0, n=65536)
    _refused(A, name + ": at most 65535 pairs a call", c, ctx, n_tri=3, n=65536)
    _refused(A, name + ": the I_0^4 table must be 4..64 knots a side", c, ctx, n_tri=3, k_=(0.0, 10.0))
    _refused(A, name + ": the I_0^4 table's k range", c, ctx, k_=(0.0, 10.0), th=F.neg)
    assert _same(ctx.covariance_ng(F.area, tri, k[0], k[1], F.ta, F.tb, knots=True), before)


def test_lds_refusals(full, big):
    """The four windows of a cross block beyond 64 kB of LDS: every call refuses by arithmetic or
    by the kernel's attributes, after its other checks and before any launch."""
    _lib, S, A, E = _lib_names()
    F, ctx = full, big.ctx
    D, n = (float(F.D[0]), float(F.D[1])), ctx.config.kernel_npoints
    o = numpy.empty(n)
    before = ctx.covariance_cross_range(), ctx.covariance_ssc_blocks_range(2)
    cross = ": halo/cosmo/window_npoints too large for the two spectra and four windows of a cross block"
    # covariance_table_cross: after the length
    _refused(A, "covariance_table_cross" + cross, ctx.covariance_table_cross, *D)
    _refused(A, "covariance_table_cross: length must be kernel_npoints", raw, ctx,
             "covariance_table_cross", D[0], D[1], P(o), None, None, n + 1)
    # covariance_blocks: after theta
    blocks = (F.code, (0, 1), F.j0, F.area, F.poisson, F.ta)
    _refused(A, "covariance_blocks" + cross, ctx.covariance_blocks, *blocks, F.tb)
    _refused(A, "covariance_blocks: theta must be positive", ctx.covariance_blocks, *blocks, -F.tb)
    # kernel_ssc_setup_cross: after the knots (and the slots, which are staged)
    ssc = (F.kt[0], F.kt[1], F.kt[2])
    _refused(A, "kernel_ssc_setup_cross: cosmo/window/corr_npoints too large for the four windows of "
                "a cross block", ctx.kernel_ssc_setup, *ssc, F.ln_chi[1], F.sigma2[1], cross=True)
    _refused(A, "kernel_ssc_setup: ln chi knots must increase", ctx.kernel_ssc_setup, *ssc,
             F.ln_chi[1][::-1], F.sigma2[1], cross=True)
    # covariance_ssc_blocks: after theta
    ssc_blocks = ((0, 1),) + ssc + (F.ln_chi, F.sigma2, F.area, F.ta)
    _refused(A, "covariance_ssc_blocks: cosmo/window/corr_npoints too large for the windows of a block",
             ctx.covariance_ssc_blocks, *ssc_blocks, F.tb)
    _refused(A, "covariance_ssc_blocks: theta must be positive", ctx.covariance_ssc_blocks,
             *ssc_blocks, -F.tb)
    assert _same((ctx.covariance_cross_range(), ctx.covariance_ssc_blocks_range(2)), before)


def test_lds_refusal_of_covariance_fourier_table(full):
    """One spectrum and the two windows of a pair: 12 (halo_npoints - 1) + 5024 doubles beside
    1824 B of static LDS pass 64 kB from halo_npoints 247 on; a context takes up to 256."""
    _lib, S, A, E = _lib_names()
    F, name = full, "covariance_fourier_table"
    ctx = Big(F, halo_npoints=256).ctx
    assert ctx.config.halo_npoints == 256
    z = numpy.linspace(0.0, 2.0, 64)
    before = ctx.covariance_fourier_zbar(z)
    ln_l = numpy.linspace(numpy.log(10.0), numpy.log(1e4), ctx.config.corr_npoints)
    _refused(A, name + ": halo/cosmo/window_npoints too large for the spectrum and the windows of a pair",
             ctx.covariance_fourier_table, F.code, [0, 1, 0, 1], ln_l)
    # precedence: the knots before the LDS
    _refused(A, name + ": ln l knots must increase", ctx.covariance_fourier_table, F.code,
             [0, 1, 0, 1], ln_l[::-1])
    assert _same(ctx.covariance_fourier_zbar(z), before)
