"""The host-side reference tests/test_gpu_devcell.py measures the device against: no GPU.
tests/test_devcell_cpu.py checks this module by itself.

* the host's plan of the C_l work buffer (cell_plan, cell_epoch_stride, cell_set_stride and
  make_proj_layout of chomp_proj_kernels.h) restated in integers;
* projection set-ups to hand in: a ProjDev's scalars and a slab of piecewise-cubic coefficients
  -- both windows, z(chi), D(z) -- each a long-double not-a-knot solve of a smooth function,
  rounded to double; the reference evaluates the same doubles;
* the chi-only node table of k_cell_nodes restated in long double: the Romberg node formula and
  its index map, the range rules of WindowView and MEView, F = w_a w_b D^2 / (D_z^2 chi^2), with a
  first-order rounding bound of what the device does with the same coefficients;
* the knot families of the product's spline tables, for the parallel not-a-knot build.
"""
import numpy

from devpower_ref import LD, EPS, U

PTAB_N = 8192
ROMBERG_DUMP = 34
CELL_TAB_LEVEL, CELL_SPLIT_LEVEL, CELL4_LEVEL, DEEP_THREADS = 16, 11, 8, 512
DEEP_LDS = 160 * 1024 - 4096
NKT = 8                                 # the kernel knots of the layout: unused by C_l, small


# -------------------------------------------------------------------------------------------
# the plan (integers)
# -------------------------------------------------------------------------------------------
def proj_layout(NC, NWp, nkt=NKT):
    """make_proj_layout: the offsets C_l reads, the total and ProjLds::doubles."""
    o, L = 0, {}
    for m in range(3):
        for name, size in (("me_z", NC), ("me_chi", NC), ("me_growth", NC),
                           ("me_pp_chi", 4 * (NC - 1)), ("me_pp_z", 4 * (NC - 1)),
                           ("me_pp_g", 4 * (NC - 1))):
            L["%s%d" % (name, m)] = o
            o += size
    for w in range(2):
        for name, size in (("w_chi", NWp), ("w_wf", NWp), ("w_pp", 4 * (NWp - 1))):
            L["%s%d" % (name, w)] = o
            o += size
    o += nkt + nkt + 4 * (nkt - 1) + nkt
    L["total"] = (o + 7) & ~7
    L["lds"] = NC + 8 * (NC - 1) + 8 * (NWp - 1)
    L["NC"], L["NWp"] = NC, NWp
    return L


def epoch_stride(n):
    return PTAB_N + 1 + n * ROMBERG_DUMP + (n + 3) // 2 + 1


def set_stride(n, LT):
    return 3 * ((1 << LT) + 1) + epoch_stride(n)


def plan(divmax, NK, NC, NWp, n, one_kernel, per_row_nodes):
    """cell_plan's fields in the order dl_plan returns them."""
    L = proj_layout(NC, NWp)
    sh_nodes = 8 * L["lds"]
    sh = 8 * 12 * (NK - 1) + sh_nodes
    shd = sh + 8 * (PTAB_N + 1)
    LT = min(divmax, CELL_TAB_LEVEL)
    split = divmax if (one_kernel > 0 or divmax <= CELL_SPLIT_LEVEL) else CELL_SPLIT_LEVEL
    four = split <= LT and split >= 6 and n >= 16
    n_nodes = (1 << LT) + 1
    stride = set_stride(n, LT) if per_row_nodes else epoch_stride(n)
    pk_at = 3 * n_nodes
    state_at = pk_at + PTAB_N + 1
    deep_at = state_at + n * ROMBERG_DUMP

    def doubles(rows):
        return (0 if per_row_nodes else 3 * n_nodes) + stride * rows
    return [sh_nodes, sh, shd, DEEP_LDS, int(shd <= DEEP_LDS), LT, split, int(four), n_nodes,
            stride, pk_at, state_at, deep_at, (n_nodes + 255) // 256, min(n, 512),
            int(bool(per_row_nodes)), doubles(1), doubles(3), epoch_stride(n), set_stride(n, LT)]


PLAN_FIELDS = ("sh_nodes", "sh", "shd", "deep_lds", "deep_fits", "LT", "split", "four", "n_nodes",
               "stride", "pk_at", "state_at", "deep_at", "gnodes", "gdeep", "per_row_nodes",
               "doubles1", "doubles3", "epoch_stride", "set_stride")


# -------------------------------------------------------------------------------------------
# the long-double not-a-knot solve (the slope system of chomp_math.h's spline_build)
# -------------------------------------------------------------------------------------------
def nak_pp(x, y):
    """pp[i, p] of sum_p pp[i, p] (x - x_i)^p, long double; tests/test_gpu_devproj.py's solve."""
    from test_gpu_devproj import nak_pp as solve
    return solve(numpy.asarray(x, dtype=LD), numpy.asarray(y, dtype=LD)[:, None])[:, :, 0]


def pp_eval(x, pp, xv, derivative=False, magnitude=False):
    """The pieces pp (any float type; evaluated in long double) on knots x at xv, each point in
    the piece a knot starts (the last piece holds the upper end and beyond, the first what lies
    below); derivative: the slope; magnitude: sum |c_p| |d|^p (of the slope: sum p |c_p| |d|^(p-1))."""
    x = numpy.asarray(x)
    xv = numpy.asarray(xv, dtype=LD)
    i = numpy.clip(numpy.searchsorted(x.astype(LD), xv, side="right") - 1, 0, x.size - 2)
    d = xv - x.astype(LD)[i]
    c = numpy.asarray(pp).astype(LD)[i]
    if magnitude:
        c, d = numpy.abs(c), numpy.abs(d)
    if derivative:
        return c[:, 1] + d * (2 * c[:, 2] + d * 3 * c[:, 3])
    return c[:, 0] + d * (c[:, 1] + d * (c[:, 2] + d * c[:, 3]))


# -------------------------------------------------------------------------------------------
# projection set-ups
# -------------------------------------------------------------------------------------------
def chi_of_z(z):
    z = numpy.asarray(z, dtype=LD)
    return LD(3000) * z * (1 - LD(0.15) * z)


def growth_of_z(z, slope=0.7):
    z = numpy.asarray(z, dtype=LD)
    return 1 / (1 + LD(slope) * z)


def bump(t):
    """(1 - t^2)^4 on [-1, 1]."""
    t = numpy.asarray(t, dtype=LD)
    return (1 - t * t) ** 4


class Proj:
    """One projection set-up: the growth / chi tables on NC uniform z in [z_lo, z_hi], the C_l
    range [chi_min, chi_max], two windows of NWp uniform chi on their own ranges wr[0], wr[1]
    (each a bump of its own height), everything else of ProjDev zero."""

    def __init__(self, NC, NWp, z_lo, z_hi, chi_min, chi_max, wr, heights=(1.3e-3, 0.8e-3),
                 slope=0.7):
        self.L = proj_layout(NC, NWp)
        self.NC, self.NWp = NC, NWp
        self.z_lo, self.z_hi, self.chi_min, self.chi_max = map(float, (z_lo, z_hi, chi_min, chi_max))
        self.wr = [(float(a), float(b)) for a, b in wr]
        self.z = numpy.linspace(self.z_lo, self.z_hi, NC)
        self.chi_k = chi_of_z(self.z).astype(float)              # the knots of z(chi): doubles
        self.pp_z = nak_pp(self.chi_k, self.z).astype(float)
        self.pp_g = nak_pp(self.z, growth_of_z(self.z, slope).astype(float)).astype(float)
        self.pp_w, self.w_x = [], []
        for (a, b), hgt in zip(self.wr, heights):
            x = numpy.linspace(a, b, NWp)
            t = numpy.linspace(-1.0, 1.0, NWp)
            self.w_x.append(x)
            self.pp_w.append(nak_pp(x, (LD(hgt) * bump(t)).astype(float)).astype(float))
        self.pdv = numpy.array([self.chi_min, self.chi_max, self.z_lo, self.z_hi, self.wr[0][0],
                                self.wr[0][1], self.wr[1][0], self.wr[1][1]])
        L = self.L
        self.tab = numpy.full(L["total"], numpy.nan)            # (what C_l never reads: NaN)
        self.tab[L["me_chi0"]:L["me_chi0"] + NC] = self.chi_k
        self.tab[L["me_pp_z0"]:L["me_pp_z0"] + 4 * (NC - 1)] = self.pp_z.ravel()
        self.tab[L["me_pp_g0"]:L["me_pp_g0"] + 4 * (NC - 1)] = self.pp_g.ravel()
        for w in range(2):
            at = L["w_pp%d" % w]
            self.tab[at:at + 4 * (NWp - 1)] = self.pp_w[w].ravel()

    # ---- the restatement: value and first-order bound of what the device makes of it ----
    def _uniform(self, x0, x1, n, pp, xv):
        """spline_eval_uniform on knots x0 + dx i, dx = (x1 - x0) / (n - 1) in double: (value,
        bound).  [derived] three fma: 3 U of sum |c_p| |d|^p; d = xv - (x0 + dx i) carries the
        rounding of the knot (product and sum: 2 U |knot|, one with an fma) and its own (U |d|),
        which move the cubic by its slope: U (3 sum |c| |d|^p + sum p |c_p| |d|^p) <= 6 U of the
        magnitude, plus 2 U |knot| of the slope's magnitude."""
        dx = (x1 - x0) / (n - 1)
        xk = LD(x0) + LD(dx) * numpy.arange(n).astype(LD)
        v = pp_eval(xk, pp, xv)
        mag = pp_eval(xk, pp, xv, magnitude=True)
        dmag = pp_eval(xk, pp, xv, derivative=True, magnitude=True)
        i = numpy.clip(numpy.searchsorted(xk, numpy.asarray(xv, dtype=LD), side="right") - 1, 0, n - 2)
        return v, 6 * LD(U) * mag + 2 * LD(U) * numpy.abs(xk[i]) * dmag

    def window(self, w, chi):
        a, b = self.wr[w]
        chi = numpy.asarray(chi, dtype=float)
        inside = (chi >= a) & (chi <= b)
        v, e = self._uniform(a, b, self.NWp, self.pp_w[w], chi)
        return numpy.where(inside, v, LD(0)), numpy.where(inside, e, LD(0)), inside

    def redshift(self, chi):
        """spline_eval on the chi knots (doubles): d = chi - x_i is one rounding."""
        v = pp_eval(self.chi_k, self.pp_z, chi)
        return v, 6 * LD(U) * pp_eval(self.chi_k, self.pp_z, chi, magnitude=True)

    def growth(self, z, dz):
        """growth_factor with its "1 outside" rule at the long-double z (its error dz moves the
        cubic by its slope)."""
        zf = numpy.asarray(z, dtype=LD)
        inside = (zf <= LD(self.z_hi)) & (zf >= LD(self.z_lo))
        v, e = self._uniform(self.z_lo, self.z_hi, self.NC, self.pp_g, zf)
        xk = LD(self.z_lo) + LD((self.z_hi - self.z_lo) / (self.NC - 1)) * numpy.arange(self.NC).astype(LD)
        e = e + numpy.abs(pp_eval(xk, self.pp_g, zf, derivative=True)) * dz
        return numpy.where(inside, v, LD(1)), numpy.where(inside, e, LD(0)), inside

    def F(self, chi, D_z):
        """(F, bound, kinds) at the doubles chi: F = (1 / D_z^2) w_a w_b D D / (chi chi).
        [derived] the cubics' bounds above through the product, 8 U of |F| for the reciprocal, the
        five products and the quotient; times two.  kinds: both windows inside, growth inside."""
        chi = numpy.asarray(chi, dtype=float)
        wa, ea, ia = self.window(0, chi)
        wb, eb, ib = self.window(1, chi)
        z, ez = self.redshift(chi)
        D, eD, ig = self.growth(z, ez)
        C = 1 / (LD(D_z) * LD(D_z)) / (chi.astype(LD) ** 2)
        F = C * wa * wb * D * D
        err = C * (ea * numpy.abs(wb) * D * D + numpy.abs(wa) * eb * D * D +
                   2 * numpy.abs(wa * wb * D) * eD) + 8 * LD(U) * numpy.abs(F)
        return F, 2 * err, (ia & ib, ig, z)


def node_index(lev, j):
    """The node table's index of the j-th new point of level lev (level 0: j = 0 -> a, 1 -> b)."""
    return j if lev == 0 else 1 + (1 << (lev - 1)) + j


def node_chi(a, b, LT):
    """The exact (a + h / 2) + h j, h = (b - a) 2^(1 - lev) (b - a in double, as the rule forms it),
    for every index of the level-LT table, in long double: (chi, level, j)."""
    N = (1 << LT) + 1
    chi = numpy.empty(N, dtype=LD)
    lev_of, j_of = numpy.zeros(N, dtype=int), numpy.zeros(N, dtype=int)
    chi[0], chi[1] = LD(a), LD(b)
    j_of[1] = 1
    rng = LD(b - a)                                             # (the double difference)
    for lev in range(1, LT + 1):
        h = rng * LD(2.0) ** (1 - lev)                          # (exact: a power of two)
        j = numpy.arange(1 << (lev - 1))
        idx = 1 + (1 << (lev - 1)) + j
        chi[idx] = (LD(a) + h / 2) + h * j.astype(LD)
        lev_of[idx], j_of[idx] = lev, j
    return chi, lev_of, j_of


def ulp(x):
    x = numpy.abs(numpy.asarray(x, dtype=float))
    return numpy.nextafter(x, numpy.inf) - x


# -------------------------------------------------------------------------------------------
# the set-ups the GPU test runs (ranges in Mpc/h; chi_of_z(0.1) = 295.5, chi_of_z(1.2) = 2952)
# -------------------------------------------------------------------------------------------
def proj_cases():
    """name -> Proj.  Window ranges: equal to [chi_min, chi_max]; strictly inside it; overhanging
    it on either side; so narrow that nodes 0, 1 and the midpoint all see zero.  `growth_ends`:
    the growth table's z range ends inside the chi range, so that growth_factor's "1 outside"
    rule is taken."""
    a, b = 400.0, 2600.0
    return {
        "equal": Proj(8, 8, 0.1, 1.2, a, b, [(a, b), (a, b)]),
        "inside": Proj(50, 100, 0.1, 1.2, a, b, [(700.0, 2100.0), (900.0, 2400.0)]),
        # (both windows reach below chi_min: the integrand does not vanish at the lower end, so a
        #  node table read one entry off shows at once)
        "overhang": Proj(50, 100, 0.1, 1.2, a, b, [(200.0, 1900.0), (150.0, 2900.0)]),
        "narrow": Proj(8, 8, 0.1, 1.2, a, b, [(a + 0.55 * (b - a), a + 0.7 * (b - a)), (a, b)]),
        "growth_ends": Proj(50, 100, 0.1, 0.8, a, b, [(a, b), (700.0, 2500.0)], slope=0.9),
    }


# -------------------------------------------------------------------------------------------
# knot families of the product's spline tables (for spline_build_pcr / spline_build_staged)
# -------------------------------------------------------------------------------------------
SPLINE_NS = (4, 5, 8, 31, 50, 63, 64, 65, 100, 128)
FAMILIES = ("ln_k", "z_chi", "chi_z", "window", "lnm_nu", "nu_lnm", "de_ln_a", "cubic")
CUBIC = (0.7, -1.3, 0.45, 0.2)          # of t = (x - x_0) / (x_n - x_0)


def family(name, n):
    """(x, y): n knots of one family, values from the oracle (the reference's algorithms)."""
    from oracle import chomp_oracle as o
    if name == "ln_k":                  # the halo-model knot tables: uniform ln k
        x = numpy.linspace(numpy.log(1e-3), numpy.log(1e2), n)
        return x, numpy.log(o.linear_power(o.epoch(), numpy.exp(x)))
    if name in ("z_chi", "chi_z"):      # MultiEpoch: chi on uniform z, and z on those chi
        e0 = o.epoch()
        z = numpy.linspace(0.05, 1.5, n)
        chi = numpy.array([o._rom(lambda zz: o.E(e0, zz), 0.0, zv, 1.48e-8, o.default_precision)
                           for zv in z])
        return (z, chi) if name == "z_chi" else (chi, z)
    if name == "window":                # a window on uniform chi
        x = numpy.linspace(350.0, 2900.0, n)
        return x, (1.3e-3 * bump(numpy.linspace(-1.0, 1.0, n))).astype(float)
    if name in ("lnm_nu", "nu_lnm"):    # the mass table: nu on uniform ln M, and ln M on those nu
        e = o.epoch()
        lnm = numpy.linspace(numpy.log(1e10), numpy.log(1e15), n)
        nu = numpy.array([o.nu_m(e, numpy.exp(v)) for v in lnm])
        return (lnm, nu) if name == "lnm_nu" else (nu, lnm)
    if name == "de_ln_a":               # the pressure table: ln a of logspace knots (de_knot)
        a = 10.0 ** numpy.linspace(numpy.log10(1.48e-8), 0.0, n)
        w0, wa = -0.9, 0.2
        return numpy.log(a), -3.0 * ((1.0 + w0 + wa) * numpy.log(a) + wa * (1.0 - a))
    if name == "cubic":                 # a cubic polynomial on non-uniform knots
        rng = numpy.random.default_rng(n)
        x = numpy.sort(numpy.concatenate([[0.0, 3.0], rng.uniform(0.0, 3.0, n - 2)]))
        x = x + 0.02 * numpy.arange(n)                          # (no two knots closer than 0.02)
        t = (x - x[0]) / (x[-1] - x[0])
        return x, CUBIC[0] + t * (CUBIC[1] + t * (CUBIC[2] + t * CUBIC[3]))
    raise KeyError(name)


# -------------------------------------------------------------------------------------------
# the C_l integrals: node values, the Romberg rows, the value's bound
# -------------------------------------------------------------------------------------------
import devpower_ref as r                                         # noqa: E402

P_LIN_BOUND = {False: 2e-13, True: 1e-12}   # [project] test_gpu_devphys.py::test_transfer_and_power
# node kinds: the table's stencil; the zero region; at_ln inside the node table -- below k_min
# (P_lin c_lo) or, without a spectrum table, the spline in range; the direct integrand beyond LT;
# at_ln's HaloFit P_mm outside [k_min, k_max]; at_ln's `extrapolate` tail above k_max
STENCIL, ZERO, AT_LN, DIRECT, AT_LN_HF, AT_LN_TAIL = range(6)
AT_KINDS = (AT_LN, AT_LN_HF, AT_LN_TAIL)
# P_lin(k_min) at z = 0 as the epochs of test_gpu_devpower.py's Case carry it (sigma_norm = 0.93 handed
# in), per (cosmology, wiggles): the one amplitude the references need.  The GPU test holds the
# device's linear spectrum to it at the [project] bound before it is used.
PLIN_KMIN = {("default", False): 4760.221661216042, ("alt", False): 6146.217613603564,
             ("default", True): 4763.550066546151}
HF_KEYS = ("k_s", "a_n", "b_n", "c_n", "alpha_n", "beta_n", "gamma_n", "mu_n", "nu_n", "f1", "f2", "f3")
HF_SET = (0.71, 1.52, 0.43, 2.1, 3.1, 1.9, 0.35, 0.0, 2.5, 1.03, 1.06, 0.93)   # test_gpu_devpower.HF_SETS[0]
TOL = 1.48e-32                          # global_precision of every case


def cell_pieces(kn):
    """The C2 family of devpower_ref.smooth_pieces, as it is: in range the spectrum is
    P_lin h_a h_b + p (HaloFit: P_mm,halofit h_a h_b + p)."""
    return r.smooth_pieces(kn)


class Spec:
    """The spectrum of a case as the C_l route sees it.  mode "mm": P_mm of the halo model (the
    spline in range, P_lin c_lo below k_min, 0 above k_max); "mm_ext": the same with `extrapolate`
    (above k_max P_lin misc[3], misc[3] = tail0 handed in: p(k_max) / P_lin(k_max), the continuous
    tail k_power_extrap would fill in for these tables); "hf_gm": HaloFit's P_gm (the spline in
    range, 0 outside); "hf_mm": HaloFit's P_mm, everywhere."""

    def __init__(self, kn, pieces, mode, bao=False, cosmo="default"):
        self.kn, self.pieces, self.mode, self.bao, self.cosmo = kn, pieces, mode, bool(bao), cosmo
        self.w = r.GM if mode == "hf_gm" else r.MM
        self.pp = pieces[r.families(self.w)[2]]
        self._plin = None

    def _ratio(self, k):
        """P_lin(k) / P_lin(k_min) by the oracle (the amplitude cancels)."""
        from oracle import chomp_oracle as o
        if self._plin is None:
            from test_gpu_devphys import COSMOS
            self._plin = o.epoch(COSMOS[self.cosmo], with_bao=self.bao)
        k = numpy.asarray(k, dtype=float)
        return (o.linear_power(self._plin, k) /
                o.linear_power(self._plin, numpy.array([r.K_MIN]))[0]).astype(LD)

    def plin(self, k):
        """The linear spectrum itself (z = 0): PLIN_KMIN times the oracle's ratio.  Against the
        device's: three [project] bounds (the device's, the oracle's, the recorded amplitude's)."""
        return LD(PLIN_KMIN[(self.cosmo, self.bao)]) * self._ratio(k)

    def _ends(self):
        """h_a h_b and p at k_min and at k_max (the pieces' end values, long double)."""
        fa, fb, fp = r.families(self.w)
        kv = r.knot_values(self.pieces, self.kn.dx).astype(LD)
        return [(kv[fa][i] * kv[fb][i], kv[fp][i]) for i in (0, -1)]

    @property
    def tail0(self):
        """misc[3] of "mm_ext", a double: P(k_max) / P_lin(k_max) = h_a h_b + p / P_lin."""
        hh, p = self._ends()[1]
        return float(hh + p / self.plin(numpy.array([r.K_MAX]))[0])

    def in_range(self, lnk):
        """(value, bound) of the evaluator at the long-double ln k: devpower_ref.in_range with the
        factor P_lin ("hf_gm": HaloFit's P_mm; "hf_mm": the HaloFit formula alone), whose own bound
        rides on the value (every term is positive)."""
        lnk = numpy.asarray(lnk, dtype=LD)
        k = numpy.exp(lnk).astype(float)
        if self.mode == "hf_mm":
            return self.halofit(k)
        idx = numpy.clip(numpy.floor((lnk - LD(self.kn.x0)) / LD(self.kn.dx)).astype(int), 0,
                         self.kn.NK - 2)
        if self.mode == "hf_gm":
            fac, fb_ = self.halofit(k)
            rel = numpy.where(fac != 0, fb_ / numpy.abs(fac).astype(float), 0.0)
        else:
            fac, rel = self.plin(k), 2 * 3 * P_LIN_BOUND[self.bao]
        v, e = r.in_range(self.w, 1.0, fac, self.pieces, self.kn, lnk, idx)
        return v, e + rel * numpy.abs(v).astype(float)

    def halofit(self, k):
        """halo.py:1339-1360 in long double on Delta^2 = P_lin k^3 / 2 pi^2 (test_gpu_devpower.py's
        mp_halofit), and test_gpu_devpower.py's halofit_bound with Delta^2 known to three [project]
        bounds of the linear spectrum (the device's, the oracle's, the recorded amplitude's)."""
        h = dict(zip(HF_KEYS, (LD(v) for v in HF_SET)))
        k = numpy.asarray(k, dtype=float)
        kl = k.astype(LD)
        pi = LD(numpy.pi) + LD(1.2246467991473532e-16)              # (pi to long double)
        dk = self.plin(k) * kl ** 3 / (2 * pi ** 2)
        assert not self.bao
        y = kl / h["k_s"]
        d2q = dk * ((1 + dk) ** h["beta_n"] / (1 + h["alpha_n"] * dk) * numpy.exp(-(y / 4 + y * y / 8)))
        d2h = (h["a_n"] * y ** (3 * h["f1"]) /
               (1 + h["b_n"] * y ** h["f2"] + (h["c_n"] * h["f3"] * y) ** (3 - h["gamma_n"]))) / \
            (1 + h["mu_n"] / y + h["nu_n"] / (y * y))
        v = 2 * pi ** 2 / kl ** 3 * (d2q + d2h)
        lk, ly, yf = numpy.abs(numpy.log(k)), numpy.abs(numpy.log(k / HF_SET[0])), k / HF_SET[0]
        args = numpy.zeros(k.size)
        for cc, L in ((HF_SET[5], numpy.abs(numpy.log1p(dk.astype(float)))), (1.0, yf / 4 + yf * yf / 8),
                      (HF_SET[9 + 1], ly), (3.0 - HF_SET[6], ly + abs(numpy.log(HF_SET[3] * HF_SET[11]))),
                      (3.0 * HF_SET[9], ly)):
            args = args + abs(cc) * (3 * U * L + r.FAST_LOG_REL * lk) + 2 * U
        rel = 2 * ((1 + abs(HF_SET[5])) * 3 * P_LIN_BOUND[False] + args + 16 * U)
        return v, rel * numpy.abs(v).astype(float)

    def outside(self, k):
        """(P, bound, kind) of the nodes with k = l / chi outside [k_min, k_max]."""
        k = numpy.asarray(k, dtype=float)
        n = k.size
        P, Pb, kind = numpy.zeros(n, dtype=LD), numpy.zeros(n), numpy.full(n, ZERO)
        lo, hi = k < r.K_MIN, k > r.K_MAX
        if self.mode == "hf_mm":
            out = lo | hi
            if out.any():
                P[out], Pb[out] = self.halofit(k[out])
                kind[out] = AT_LN_HF
        if self.mode in ("mm", "mm_ext") and lo.any():
            # P_lin(k) c_lo, c_lo = h_a h_b + p / P_lin at k_min: two linear spectra, three [project]
            # bounds each, times two
            hh, p0 = self._ends()[0]
            v = self.plin(k[lo]) * (hh + p0 / self.plin(numpy.array([r.K_MIN]))[0])
            P[lo], Pb[lo], kind[lo] = v, 2 * 6 * P_LIN_BOUND[self.bao] * numpy.abs(v).astype(float), AT_LN
        if self.mode == "mm_ext" and hi.any():
            # P_lin(k) misc[3]: three [project] bounds, times two
            v = LD(self.tail0) * self.plin(k[hi])
            P[hi], Pb[hi], kind[hi] = v, 2 * 3 * P_LIN_BOUND[self.bao] * numpy.abs(v).astype(float), AT_LN_TAIL
        return P, Pb, kind

    def table(self, x0, x1):
        """k_cell_ptab's table from the reference alone (the CPU test's stand-in for the read-back
        one): the spectrum at x0 + (x1 - x0) (i / kPTabN), the ends at x0 and x1."""
        x = LD(x0) + (LD(x1) - LD(x0)) * (numpy.arange(PTAB_N + 1) / float(PTAB_N)).astype(LD)
        return self.in_range(x)[0].astype(float)


def stencil_indices(u):
    """devpower_ref.stencil_index (from_table's interval choice) per node."""
    return numpy.array([r.stencil_index(float(v), PTAB_N)[1] for v in u], dtype=int)


def lagrange6(q, t):
    """devpower_ref.lagrange6 on arrays: q[m] the six table values per node, t per node."""
    return r.lagrange6(q, numpy.asarray(t, dtype=LD))


class Tables:
    """What the kernels read besides the spline pieces: the node table of level LT (F, ln chi,
    chi), the spectrum table, the device's logarithms.  host(): the reference's own stand-ins."""

    def __init__(self, LT, F, lnchi, chi, pk, x0, x1, ln_ell):
        self.LT, self.F, self.lnchi, self.chi, self.pk = LT, F, lnchi, chi, pk
        self.x0, self.x1, self.ln_ell = float(x0), float(x1), numpy.asarray(ln_ell, dtype=float)
        self.pdx = (self.x1 - self.x0) / float(PTAB_N)
        self.pinv = 1.0 / self.pdx

    @classmethod
    def host(cls, case):
        chi = node_chi(case.proj.chi_min, case.proj.chi_max, case.LT)[0].astype(float)
        F = case.proj.F(chi, case.D_z)[0].astype(float)
        x0, x1 = float(numpy.log(r.K_MIN)), float(numpy.log(r.K_MAX))
        pk = case.spec.table(x0, x1) if case.use_ptab else None
        return cls(case.LT, F, numpy.log(chi), chi, pk, x0, x1, numpy.log(case.ell))


class CellCase:
    """One launch's inputs: projection set-up, D_z, spectrum, multipoles, rule and levels."""

    def __init__(self, name, proj, spec, ell, rtol, divmax, LT, split, D_z=0.77, use_ptab=True):
        self.name, self.proj, self.spec, self.D_z = name, proj, spec, D_z
        self.ell = numpy.asarray(ell, dtype=float)
        self.rtol, self.divmax, self.LT, self.split, self.use_ptab = rtol, divmax, LT, split, use_ptab

    # ---- node values of one multipole at one level: (f, bound, kind) ----
    def level_nodes(self, T, il, lev):
        ell, a, b = self.ell[il], self.proj.chi_min, self.proj.chi_max
        if lev <= T.LT:
            idx = numpy.array([0, 1]) if lev == 0 else 1 + (1 << (lev - 1)) + numpy.arange(1 << (lev - 1))
            return self._table_nodes(T, il, idx)
        h = (b - a) * 2.0 ** (1 - lev)
        chi = (a + 0.5 * h) + h * numpy.arange(1 << (lev - 1))
        return self._direct_nodes(ell, chi)

    def _outside(self, k, n):
        """Nodes the spline does not answer, by k = l / chi: (P, bound, kind)."""
        return self.spec.outside(k)

    def _table_nodes(self, T, il, idx):
        ell = self.ell[il]
        F, k = T.F[idx], ell / T.chi[idx]
        lk = T.ln_ell[il] - T.lnchi[idx]                         # (the device's own doubles)
        P, Pb, kind = self._outside(k, idx.size)
        inr = (k >= r.K_MIN) & (k <= r.K_MAX)
        if T.pk is not None:
            u = (lk - T.x0) * T.pinv
            ins = (u >= 0.0) & (u <= float(PTAB_N))
            # from_table and at_ln decide the range by u and by k: the cases keep both off the ends
            assert numpy.array_equal(ins, inr), "a node within rounding of k_min or k_max"
            i = stencil_indices(u)
            t = u - i
            q = [T.pk[i - 2 + m] for m in range(6)]
            v, s = lagrange6(q, t)
            v = numpy.where(u == float(PTAB_N), q[5].astype(LD), v)
            P = numpy.where(ins, v, P)
            # [derived] K_STENCIL U sum |q_m L_m(t)|, times two
            Pb = numpy.where(ins, 2 * r.K_STENCIL * U * s.astype(float), Pb)
            kind = numpy.where(ins, STENCIL, kind)
        elif inr.any():                                           # at_ln at every node
            v, e = self.spec.in_range(lk[inr].astype(LD))
            P[inr], Pb[inr], kind[inr] = v, e, AT_LN
        f = P * F.astype(LD)
        return f, Pb * numpy.abs(F) + U * numpy.abs(f).astype(float), kind

    def _direct_nodes(self, ell, chi):
        """Beyond the table: eval_t(l / chi) times the windows and the growth at chi itself; chi
        within an ulp of the device's (lox + h j, with or without an fma): F and P move by their
        change over two ulps."""
        k = ell / chi
        P, Pb, _ = self._outside(k, chi.size)
        inr = (k >= r.K_MIN) & (k <= r.K_MAX)
        if inr.any():
            lnk = numpy.log(k[inr].astype(LD))
            v, e = self.spec.in_range(lnk)
            v2 = self.spec.in_range(lnk + 4 * LD(EPS))[0]
            P[inr], Pb[inr] = v, e + numpy.abs(v2 - v).astype(float)
        F, Fb, _ = self.proj.F(chi, self.D_z)
        F2 = self.proj.F(chi + 2 * ulp(chi), self.D_z)[0]
        Fb = Fb.astype(float) + numpy.abs(F2 - F).astype(float)
        f = P * F
        bound = Pb * numpy.abs(F).astype(float) + numpy.abs(P).astype(float) * Fb + 4 * U * numpy.abs(f).astype(float)
        return f, bound, numpy.full(chi.size, DIRECT)

    # ---- the rule ----
    def reference(self, T, il, upto=None):
        """scipy.integrate.romberg's rows (oracle/romberg.py) replayed in long double on the node
        values above, to the stopping level and one beyond (for the neighbouring row).  The
        quadrature R[i][i] has positive weights, so the same rows on the nodes' bounds carry them
        to the value exactly; the rows' own rounding: [project] 16 eps |b - a| mean |f|
        (test_gpu_romberg.py).  Returns a dict: level, converged, value, bound, rows, row_bounds,
        T (trapezoid estimates), ordsum (after each level), margins (err / (rtol |cur|) per
        decision), kinds (node kinds met up to the stopping level)."""
        a, b = self.proj.chi_min, self.proj.chi_max
        rng = LD(b - a)
        f, e, kind = self.level_nodes(T, il, 0)
        ordsum, esum, asum, count = f.sum() / 2, e.sum() / 2, numpy.abs(f).sum(), 2
        last, elast = [rng * ordsum], [float(rng) * esum]
        out = dict(rows=[last[0]], row_bounds=[elast[0]], T=[last[0]], T_bounds=[elast[0]],
                   ordsum=[ordsum], ordsum_bounds=[esum], margins=[],
                   kinds=set(kind.tolist()), level=None, converged=False, fast_fails=False)
        stop = None
        top = self.divmax if upto is None else upto
        for i in range(1, top + 1):
            f, e, kind = self.level_nodes(T, il, i)
            ordsum, esum, asum, count = ordsum + f.sum(), esum + e.sum(), asum + numpy.abs(f).sum(), count + f.size
            row, erow = [rng * ordsum / 2 ** i], [float(rng) * esum / 2 ** i]
            for k in range(i):
                tmp = LD(4) ** (k + 1)
                row.append((tmp * row[k] - last[k]) / (tmp - 1))
                erow.append((float(tmp) * erow[k] + elast[k]) / (float(tmp) - 1))
            cur, err = row[i], abs(row[i] - last[i - 1])
            rows_b = 16 * EPS * float(rng) * float(asum) / count
            out["rows"].append(cur)
            # (R[i][i] = sum_m C[i][m] T_m: the same recurrence on the bounds of the T_m with every
            #  sign dropped is sum_m |C[i][m]| bound(T_m), at most 1.94 times the largest)
            out["row_bounds"].append(erow[i] + rows_b)
            out["T"].append(row[0])
            out["T_bounds"].append(erow[0] + rows_b)
            out["ordsum"].append(ordsum)
            out["ordsum_bounds"].append(esum + 16 * EPS * float(asum))
            if stop is None:
                out["kinds"] |= set(kind.tolist())
                if i > self.split and i <= T.LT and T.pk is not None:
                    # a k_cell_deep batch (four nodes 512 apart) with a node fast() refuses
                    n4 = (f.size // 2048) * 2048
                    if n4:
                        ok = (~numpy.isin(kind[:n4], AT_KINDS)).reshape(-1, 4, 512)
                        out["fast_fails"] |= bool(numpy.any(~ok.all(axis=1) & ok.any(axis=1)))
                if err == 0 and cur == 0:
                    out["margins"].append(0.0)
                else:
                    out["margins"].append(float(err / (LD(self.rtol) * abs(cur))))
                if err < TOL or err < LD(self.rtol) * abs(cur):
                    stop = i
                    out.update(level=i, converged=True)
            elif i > stop:
                break
            last, elast = row, erow
        if stop is None:
            out["level"] = top
        s = out["level"]
        out["value"], out["bound"] = out["rows"][s], out["row_bounds"][s]
        return out


def pins_the_level(ref):
    """The two conditions under which the value pins the stopping level: (a) every decision at
    least 1e3 (bound / |value|) from its threshold; (b) the rows at the stopping level and its
    neighbours more than 8 bounds apart.  (A value of exactly 0 from all-zero nodes: exact.)"""
    s, v, B = ref["level"], ref["value"], ref["bound"]
    if v == 0 and B == 0:
        return True, True
    rel = 1e3 * B / abs(float(v))
    a_ok = all(abs(m - 1.0) >= rel for m in ref["margins"][:s])
    rows = ref["rows"]
    b_ok = abs(rows[s] - rows[s - 1]) > 8 * B and (s + 1 >= len(rows) or abs(rows[s + 1] - rows[s]) > 8 * B)
    return a_ok, b_ok


# -------------------------------------------------------------------------------------------
# the launches the GPU test runs
# -------------------------------------------------------------------------------------------
def multipoles(n=40):
    """40 multipoles: 8 where l / chi crosses k_min inside the chi range (nodes at_ln answers), 8
    where every node reads the table, 24 where l / chi crosses k_max (the spectrum's cut: nodes in
    the zero region, the slow integrals; the highest see zero at nodes 0, 1 and the midpoint).  n <
    40: a spread of them."""
    ell = numpy.concatenate([numpy.logspace(numpy.log10(0.3), numpy.log10(3.0), 8),
                             numpy.logspace(1, 4, 8),
                             numpy.logspace(numpy.log10(3e4), numpy.log10(2.7e5), 24)])
    return ell if n == 40 else ell[numpy.round(numpy.linspace(0, 39, n)).astype(int)]


K_LEAN, K_DIRECT, K_FOUR = 0, 1, 2       # k_cell<.., false>, k_cell<.., true>, k_cell4
# name: (proj, NK, mode, bao, use_ptab, n_ell, rtol, divmax, LT, split, kind, deep blocks)
LAUNCHES = {
    # 2. k_cell alone, split = divmax
    "cell_lean": ("equal", 8, "mm", 0, 1, 40, 1.48e-4, 12, 12, 12, K_LEAN, 0),
    "cell_direct": ("growth_ends", 50, "mm", 0, 1, 40, 1.48e-4, 12, 9, 12, K_DIRECT, 0),
    "cell_hf": ("inside", 50, "hf_gm", 0, 1, 40, 1.48e-5, 12, 9, 12, K_DIRECT, 0),
    "cell_bao": ("overhang", 8, "mm", 1, 0, 40, 1.48e-4, 12, 9, 12, K_DIRECT, 0),
    # 3. - 5. k_cell4 / k_cell, the hand-over, k_cell_deep
    "four_11": ("growth_ends", 50, "mm", 0, 1, 40, 1.48e-5, 12, 12, 11, K_FOUR, 40),
    "four_8": ("growth_ends", 8, "mm", 0, 1, 16, 1.48e-5, 12, 9, 8, K_FOUR, 1),
    "four_6": ("inside", 50, "mm", 0, 1, 17, 1.48e-5, 12, 12, 6, K_FOUR, 3),
    "four_all_11": ("overhang", 50, "mm", 0, 1, 18, 1.48e-6, 11, 11, 11, K_FOUR, 0),
    "four_all_8": ("equal", 8, "mm", 0, 1, 19, 1.48e-3, 8, 9, 8, K_FOUR, 0),
    "four_hf": ("inside", 50, "hf_gm", 0, 1, 40, 1.48e-5, 12, 12, 11, K_FOUR, 40),
    "cell_hand": ("equal", 50, "mm", 0, 1, 40, 1.48e-5, 12, 9, 9, K_DIRECT, 3),
    "lean_hand": ("overhang", 8, "mm", 0, 1, 40, 1.48e-6, 12, 12, 11, K_LEAN, 1),
    # at_ln's other branches as nodes of the table: HaloFit's P_mm outside [k_min, k_max] on both
    # sides, and the `extrapolate` tail above k_max, each handed on to k_cell_deep
    "hf_mm_hand": ("growth_ends", 50, "hf_mm", 0, 1, 40, 1.48e-5, 12, 12, 11, K_FOUR, 40),
    "hf_mm_direct": ("growth_ends", 8, "hf_mm", 0, 1, 40, 1.48e-5, 12, 9, 9, K_DIRECT, 3),
    "ext_hand": ("growth_ends", 50, "mm_ext", 0, 1, 40, 1.48e-5, 12, 12, 11, K_FOUR, 40),
    # wiggles: k_cell4<false, true> and k_cell_deep<false, true> without a spectrum table (fast()
    # refuses every batch)
    "four_bao": ("overhang", 8, "mm", 1, 0, 40, 1.48e-5, 12, 12, 11, K_FOUR, 3),
    "ext_direct": ("overhang", 8, "mm_ext", 0, 1, 40, 1.48e-6, 12, 9, 9, K_DIRECT, 3),
}
FIELDS = ("proj", "NK", "mode", "bao", "use_ptab", "n", "rtol", "divmax", "LT", "split", "kind", "blocks")


def launch(name, kn=None, pieces=None, projs=None):
    """(CellCase, the launch's fields) of one entry of LAUNCHES; kn / pieces: the device's knots
    and the pieces handed in (the GPU test), else numpy's logarithms and cell_pieces."""
    L = dict(zip(FIELDS, LAUNCHES[name]))
    kn = r.Knots(L["NK"]) if kn is None else kn
    pieces = cell_pieces(kn) if pieces is None else pieces
    projs = proj_cases() if projs is None else projs
    case = CellCase(name, projs[L["proj"]], Spec(kn, pieces, L["mode"], L["bao"]), multipoles(L["n"]),
                    L["rtol"], L["divmax"], L["LT"], L["split"], use_ptab=bool(L["use_ptab"]))
    return case, L


# the _epochs (form 1) and _sets (form 2) runs: 3 rows each
ROW_RUNS = ((1, "four_11"), (1, "cell_hand"), (2, "four_6"), (2, "cell_hand"))
SET_PROJS, SET_DZ = ("inside", "growth_ends", "overhang"), (0.77, 0.61, 0.93)
ROW_COSMOS = ("default", "alt", "default")                      # epochs A B A


def row_scale(y):
    return 1.0 + 0.1 * (y % 2)


def row_case(form, name, y, kn=None, pieces=None, projs=None):
    """Row y of a run of ROW_RUNS as a CellCase: epoch y (cosmology ROW_COSMOS[y], the pieces
    scaled by row_scale(y)) on the launch's own projection (form 1) or on set y (form 2)."""
    L = dict(zip(FIELDS, LAUNCHES[name]))
    kn = r.Knots(L["NK"]) if kn is None else kn
    pieces = cell_pieces(kn) * row_scale(y) if pieces is None else pieces
    projs = proj_cases() if projs is None else projs
    proj = projs[SET_PROJS[y]] if form == 2 else projs[L["proj"]]
    D = SET_DZ[y] if form == 2 else 0.77
    return CellCase("%s form %d row %d" % (name, form, y), proj,
                    Spec(kn, pieces, L["mode"], L["bao"], ROW_COSMOS[y]), multipoles(L["n"]), L["rtol"],
                    L["divmax"], L["LT"], L["split"], D_z=D), L
