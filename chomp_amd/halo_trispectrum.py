"""halo_trispectrum.HaloTrispectrumOneHalo (halo_trispectrum.py:13-151) over the HIP library: the
one-halo term of the matter (or galaxy) trispectrum,

    I_0^4(k1, k2, k3, k4) = int nu f(nu) y(k1, M) y(k2, M) y(k3, M) y(k4, M) M^3 n(M) dln nu
                            / rho_bar^3,

with n(M) the HOD moment power_spec selects.  i_0_4 / trispectrum / i_0_4_many run one Romberg per
quadruple on the device (k_tri1h_quad); trispectrum_parallelogram builds the reference's 50 x 50
table of I_0^4(k_i, k_i, k_j, k_j) and its bicubic spline in one set-up (k_tri1h_table,
k_tri1h_bicubic) and evaluates the spline there.

Kept as shipped:

* the result of trispectrum_parallelogram is grid-shaped (scalars give a 1 x 1 array); k < k_min
  is clamped to k_min and the spline clamps to the knot range on its own; the k_max mask is
  applied with numpy's broadcasting, so for 1-D arguments it zeroes COLUMNS (j where k1[j] or
  k2[j] > k_max) while a row with k1 > k_max keeps spline values;
* the constructor replaces the Halo's HOD (local_hod) without the set_hod_object bookkeeping;
* set_cosmology (and set_redshift through it) moves the halo model first and then calls
  self.pert.set_cosmology_object: with the default perturbation=None that raises AttributeError
  and _initialized_i_0_4 stays True, so the table of the first build keeps being served.  The
  table lives in a device context of its own, which is what keeps it there;
* the integral runs from nu_min whatever the HOD's moment zeros are, on the unnormalised
  integrand (the reference computes a lower limit and a norm and uses neither).

Outside the device's scope (ChompScopeError): an HOD other than HODZheng / HODMandelbaum, and
halo alpha != -1 (as for Halo).  Not kept: the reference's Halo.__init__ computes n_bar with a
default HODZheng before local_hod is replaced; here power_gm / power_gg of this object use
local_hod throughout.

HaloTrispectrum (halo_trispectrum.py:153-837), the two- to four-halo terms, is documented at the
class.
"""
import warnings

import numpy

from . import _lib
from . import cosmology
from . import halo
from . import hod


def _quads(k):
    if _lib._is_torch(k):
        if k.dim() != 2 or k.shape[1] != 4:
            raise ValueError("quadruples are an (N, 4) array, got shape %r" % (tuple(k.shape),))
        return k
    v = numpy.asarray(k, dtype=numpy.float64)
    if v.ndim != 2 or v.shape[1] != 4:
        raise ValueError("quadruples are an (N, 4) array, got shape %r" % (v.shape,))
    return v


class HaloTrispectrumOneHalo(halo.Halo):
    """The one-halo term of the trispectrum (halo_trispectrum.py:13-151)."""

    def __init__(self, redshift=0.0, single_epoch_cosmo=None, mass_func_second=None,
                 perturbation=None, halo_dict=None, input_hod=None, power_spec='power_mmmm'):
        self.pert = perturbation
        halo.Halo.__init__(self, redshift, None, single_epoch_cosmo, mass_func_second, halo_dict)
        self.power_spec = power_spec
        if input_hod is None:
            input_hod = hod.HODZheng()
        if not isinstance(input_hod, (hod.HODZheng, hod.HODMandelbaum)):
            raise _lib.ChompScopeError(
                "HaloTrispectrumOneHalo: the device models HODZheng and HODMandelbaum only, "
                "not %s" % type(input_hod).__name__)
        halo._check_hod(input_hod)
        self.local_hod = input_hod
        self._initialized_i_0_4 = False
        self._tri_ctx = None

    def _moment(self):
        return _lib.TRI_MOMENT.get(self.power_spec, 0)

    def set_cosmology(self, cosmo_dict, redshift=None):
        """halo_trispectrum.py:29-46."""
        if redshift is None:
            redshift = self._redshift
        halo.Halo.set_cosmology(self, cosmo_dict, redshift)
        self.pert.set_cosmology_object(self.cosmo)
        self._initialized_i_0_4 = False

    def trispectrum(self, k1, k2, k3, k4):
        return self.i_0_4(k1, k2, k3, k4)

    def trispectrum_parallelogram(self, k1, k2):
        if not self._initialized_i_0_4:
            self._initialize_i_0_4()
        return self.i_0_4_parallelogram(k1, k2)

    def i_0_4(self, k1, k2, k3, k4):
        """halo_trispectrum.py:60-95 at one quadruple of scalars."""
        k = numpy.array([[k1, k2, k3, k4]], dtype=numpy.float64)
        return numpy.float64(self._quad_host(k)[0])

    def i_0_4_many(self, k):
        """i_0_4 at every row of k, an (N, 4) array or a contiguous float64 torch cuda tensor
        (then on the device without a host round trip, asynchronous on the context's stream; the
        result is a tensor)."""
        k = _quads(k)
        if _lib._is_torch(k):
            ctx = self._sync(0, defer_status=True)
            return ctx.tri1h_quad(self._moment(), k.contiguous(), 0)
        return self._quad_host(k)

    def _quad_host(self, k):
        ctx = self._sync(0)
        out = ctx.tri1h_quad(self._moment(), k, 0)
        if ctx.status(0, 1)[0] & _lib.ST_TRI1H_DIVMAX:
            warnings.warn("i_0_4: " + "; ".join(_lib.describe_status(_lib.ST_TRI1H_DIVMAX)),
                          _lib.ChompAccuracyWarning, stacklevel=3)
        return out

    def i_0_4_parallelogram(self, k1, k2):
        """halo_trispectrum.py:97-102."""
        k1 = numpy.where(k1 < self._k_min, self._k_min, k1)
        k2 = numpy.where(k2 < self._k_min, self._k_min, k2)
        return numpy.where(
            numpy.logical_and(k1 <= self._k_max, k2 <= self._k_max),
            self._i_0_4_spline(numpy.log(k1), numpy.log(k2)),
            0.0)

    def _i_0_4_spline(self, x, y):
        """RectBivariateSpline.__call__(x, y) (grid=True) of the table: shape (x.size, y.size),
        the arguments sorted, each clamped into the knot range."""
        if self._tri_ctx is None:
            raise AttributeError("'HaloTrispectrumOneHalo' object has no attribute "
                                 "'_i_0_4_spline'")
        x = numpy.atleast_1d(numpy.asarray(x, dtype=numpy.float64))
        y = numpy.atleast_1d(numpy.asarray(y, dtype=numpy.float64))
        for name, v in (("x", x), ("y", y)):
            if v.ndim != 1:
                raise ValueError("%s must be a 1-D array" % name)
            if v.size >= 2 and not numpy.all(numpy.diff(v) >= 0.0):
                raise ValueError("%s must be strictly increasing" % name)
        a, b = numpy.meshgrid(x, y, indexing="ij")
        return self._tri_ctx.tri1h_eval(a, b, 0).reshape(x.size, y.size)

    def _initialize_i_0_4(self):
        """halo_trispectrum.py:104-129: the table, its Romberg levels and its bicubic, in a
        context that holds this halo model's epoch as it is now."""
        if self._tri_ctx is None:
            self._tri_ctx = cosmology._context()
        ctx = self._tri_ctx
        bao = bool(getattr(self.cosmo, "_with_bao", False))
        ctx.epochs_set(self.cosmo.cosmo_dict, [self.cosmo._redshift], bao,
                       **cosmology._de_kw(self.cosmo.cosmo_dict))
        ctx.stage_k(self.mass.halo_dict, self.mass._kind, self._profile(), self.local_hod, 0)
        tab, lev = ctx.tri1h_setup(self._moment(), 0, 1, copy_out=True)
        ctx.warn_status(0, 1, stacklevel=4)
        self._i_0_4_array = tab[0]
        self._i_0_4_levels = lev[0]
        self._initialized_i_0_4 = True


_TABLES = ("i_0_4", "i_1_2", "i_1_3", "i_2_1", "i_2_2")
_NAN_MSG = ("%s: the reference serves NaN here (its table's diagonal is the k1 = k2 angle "
            "integral, whose theta = 0 end point is not finite, halo_trispectrum.py:%s): outside "
            "the accelerated scope; tri_spec_proj_integral(k1, k2) with k1 != k2 is built")


def _rows(a, width, what):
    if _lib._is_torch(a):
        if a.dim() != 2 or a.shape[1] != width:
            raise ValueError("%s are an (N, %d) array, got shape %r"
                             % (what, width, tuple(a.shape)))
        return a.contiguous()
    v = numpy.asarray(a, dtype=numpy.float64)
    if v.ndim != 2 or v.shape[1] != width:
        raise ValueError("%s are an (N, %d) array, got shape %r" % (what, width, v.shape))
    return v


class HaloTrispectrum(halo.Halo):
    """The two- to four-halo terms of the matter trispectrum of a parallelogram
    (halo_trispectrum.py:153-837, Cooray & Hu 2001): T(k1, k2, z) with z the cosine between k1
    and k2.  The five mass-integral tables are built in one device set-up (k_tri1h_table,
    k_tri_table, k_tri_finish); t_1_h .. t_4_h run in k_tri_terms and tri_spec_proj_integral in
    k_tri_proj.  terms_many / tri_spec_proj_integral_many are the batch entry points (no
    counterpart in the reference, which takes scalar k1, k2).

    Kept as shipped: _i_1_3 is mirrored from I(k_i, k_i, k_j), i <= j; _i_2_2's integrand reads
    y(k_j)^2; _i_2_1 is Romberg of the raw integrand times the integrand at ln nu = 0; t_3_h's
    perm_4 uses the unguarded bispectrum; look-ups clamp k < k_min to k_min and give 0 above
    k_max; the constructor never hands the halo's cosmology to `perturbation`, so the PT forms use
    whatever cosmology and redshift that object has until set_cosmology realigns it;
    tri_spec_proj_integral(k, k) is NaN (and raises the CHOMP_ST_TRI_DIVMAX status bit).

    Outside the scope (ChompScopeError): a mass function without bias_2_nu (the reference ends in
    AttributeError inside t_3_h / t_4_h), trispectrum_projected and t_PT_averaged (NaN as
    shipped).  Covariance does not take this class (it calls trispectrum_parallelogram(ka, kb))."""

    def __init__(self, redshift=0.0, single_epoch_cosmo=None, mass_func_second=None,
                 perturbation=None, halo_dict=None):
        from . import mass_function
        from . import perturbation_spectra
        if not isinstance(mass_func_second, mass_function.MassFunctionSecondOrder):
            raise _lib.ChompScopeError(
                "HaloTrispectrum (the two- to four-halo trispectrum terms) is outside the "
                "accelerated scope without a second-order mass function; HaloTrispectrumOneHalo "
                "is built.  To opt in pass mass_func_second=MassFunctionSecondOrder(redshift, "
                "cosmo): t_3_h and t_4_h need its bias_2_nu")
        if perturbation is None:
            perturbation = perturbation_spectra.PerturbationTheory()
        self.pert = perturbation
        halo.Halo.__init__(self, redshift, None, single_epoch_cosmo, mass_func_second, halo_dict)
        self._tri_ctx = None
        self._tri_sig = None
        self._pt_epoch = 0
        self._reset_tri_flags()

    def _reset_tri_flags(self):
        for name in _TABLES:
            setattr(self, "_initialized_" + name, False)
        self._initialzied_PT_averaged = False
        self._initialized_tri_proj = False
        self._tables_built = False

    def set_cosmology(self, cosmo_dict, redshift=None):
        """halo_trispectrum.py:201-224."""
        if redshift is None:
            redshift = self._redshift
        halo.Halo.set_cosmology(self, cosmo_dict, redshift)
        self.pert.set_cosmology_object(self.cosmo)
        self._reset_tri_flags()

    def set_redshift(self, redshift):
        """halo_trispectrum.py:226-234."""
        self.set_cosmology(self.cosmo.cosmo_dict, redshift)

    # -- device ------------------------------------------------------------------
    def _device(self):
        """The context of the tables: epoch 0 is the halo model's, epoch 1 (when it differs) the
        PerturbationTheory object's; (re)built when either object has moved."""
        pc = self.pert.cosmo
        bao = bool(getattr(self.cosmo, "_with_bao", False))
        if bool(getattr(pc, "_with_bao", False)) != bao:
            raise _lib.ChompScopeError(
                "HaloTrispectrum: the halo model and the PerturbationTheory object use "
                "different transfer functions (with_bao)")
        he = (tuple(sorted(self.cosmo.cosmo_dict.items())), self.cosmo._redshift)
        pe = (tuple(sorted(pc.cosmo_dict.items())), pc._redshift)
        sig = (he, pe, bao, tuple(sorted(self.mass.halo_dict.items())), self.mass._kind,
               tuple(sorted(self._profile().items())))
        if self._tri_ctx is None:
            self._tri_ctx = cosmology._context()
            self._tri_ctx.set_second_order(True)
        ctx = self._tri_ctx
        if sig != self._tri_sig or not self._tables_built:
            cosmos = [self.cosmo.cosmo_dict] + ([pc.cosmo_dict] if pe != he else [])
            zs = [self.cosmo._redshift] + ([pc._redshift] if pe != he else [])
            ctx.epochs_set(_lib.Context.pack_cosmo(cosmos, len(cosmos)), zs, bao,
                           **cosmology._de_kw(cosmos))
            ctx.stage_k(self.mass.halo_dict, self.mass._kind, self._profile(), self.local_hod,
                        _lib.T_H_M)
            tab, lev = ctx.tri_setup(0, 1, copy_out=True)
            ctx.warn_status(0, 1, stacklevel=5)
            self._tri_tables = {k: v[0] for k, v in tab.items()}
            self._tri_levels = {k: v[0] for k, v in lev.items()}
            self._pt_epoch = len(zs) - 1
            self._tri_sig = sig
            self._tables_built = True
            self._initialized_h_m = True
        return ctx

    def _initialize(self, name):
        self._device()
        setattr(self, "_%s_array" % name, self._tri_tables[name])
        setattr(self, "_%s_levels" % name, self._tri_levels[name])
        setattr(self, "_initialized_" + name, True)

    def _initialize_i_0_4(self):
        self._initialize("i_0_4")

    def _initialize_i_1_2(self):
        self._initialize("i_1_2")

    def _initialize_i_1_3(self):
        self._initialize("i_1_3")

    def _initialize_i_2_1(self):
        self._initialize("i_2_1")

    def _initialize_i_2_2(self):
        self._initialize("i_2_2")

    def _ready(self, names=_TABLES):
        for name in names:
            if not getattr(self, "_initialized_" + name):
                self._initialize(name)
        return self._device()

    def _lookup(self, name, k1, k2):
        ctx = self._ready(() if name == "i_1_1" else (name,))
        a, b = numpy.broadcast_arrays(numpy.asarray(k1, dtype=numpy.float64),
                                      numpy.asarray(k2, dtype=numpy.float64))
        out = ctx.tri_table_eval(name, a.ravel(), b.ravel(), 0).reshape(a.shape)
        return out if a.shape else numpy.float64(out)

    # -- batch entry points ----------------------------------------------------------
    def terms_many(self, kkz):
        """t_1_h, t_2_h, t_3_h, t_4_h [N, 4] at the rows (k1, k2, z) of kkz, an (N, 3) array or a
        contiguous float64 torch cuda tensor (then on the device without a host round trip,
        asynchronous on the context's stream; the result is a tensor)."""
        kkz = _rows(kkz, 3, "configurations (k1, k2, z)")
        return self._ready().tri_terms(kkz, 0, self._pt_epoch)

    def tri_spec_proj_integral_many(self, kk, levels=False):
        """tri_spec_proj_integral at the rows (k1, k2) of kk, an (N, 2) array or a contiguous
        float64 torch cuda tensor.  levels: also the Romberg levels and the NaN / divmax flags."""
        kk = _rows(kk, 2, "pairs (k1, k2)")
        ctx = self._ready()
        if _lib._is_torch(kk):
            return ctx.tri_proj(kk, 0, self._pt_epoch, levels=levels)
        # (the status bit stays up until the next set-up: this call's own flags decide)
        out, lev, flag = ctx.tri_proj(kk, 0, self._pt_epoch, levels=True)
        if numpy.any(flag != 0.0):
            warnings.warn("tri_spec_proj_integral: " +
                          "; ".join(_lib.describe_status(_lib.ST_TRI_DIVMAX)),
                          _lib.ChompAccuracyWarning, stacklevel=3)
        return (out, lev, flag) if levels else out

    def _terms(self, k1, k2, z):
        k1, k2, z = numpy.broadcast_arrays(*[numpy.asarray(v, dtype=numpy.float64)
                                             for v in (k1, k2, z)])
        out = self.terms_many(numpy.stack([k1.ravel(), k2.ravel(), z.ravel()], axis=1))
        return out, k1.shape

    def _term(self, col, k1, k2, z):
        out, shape = self._terms(k1, k2, z)
        return out[:, col].reshape(shape) if shape else numpy.float64(out[0, col])

    # -- reference surface -------------------------------------------------------------
    def trispectrum_parallelogram(self, k1, k2, z):
        """halo_trispectrum.py:236-254: t_1_h + t_2_h + t_3_h + t_4_h."""
        out, shape = self._terms(k1, k2, z)
        s = ((out[:, 0] + out[:, 1]) + out[:, 2]) + out[:, 3]
        return s.reshape(shape) if shape else numpy.float64(s[0])

    def t_1_h(self, k1, k2):
        return self.i_0_4_parallelogram(k1, k2)

    def t_2_h(self, k1, k2, z):
        return self._term(1, k1, k2, z)

    def t_3_h(self, k1, k2, z):
        return self._term(2, k1, k2, z)

    def t_4_h(self, k1, k2, z):
        return self._term(3, k1, k2, z)

    def t_PT(self, k1, k2, z):
        return self.pert.trispectrum_parallelogram(k1, k2, z)

    def tri_spec_proj_integral(self, k1, k2):
        """halo_trispectrum.py:267-278 at one pair of scalars; NaN for k1 = k2."""
        kk = numpy.array([[k1, k2]], dtype=numpy.float64)
        return numpy.float64(self.tri_spec_proj_integral_many(kk)[0])

    def trispectrum_projected(self, k1, k2):
        raise _lib.ChompScopeError(_NAN_MSG % ("trispectrum_projected", "256-313"))

    def _initialize_tri_proj(self):
        raise _lib.ChompScopeError(_NAN_MSG % ("_initialize_tri_proj", "280-313"))

    def t_PT_averaged(self, k1, k2):
        raise _lib.ChompScopeError(_NAN_MSG % ("t_PT_averaged", "517-559"))

    def _initialize_PT_averaged(self):
        raise _lib.ChompScopeError(_NAN_MSG % ("_initialize_PT_averaged", "528-559"))

    def i_0_4(self, k1, k2, k3, k4):
        """halo_trispectrum.py:566-583 at one quadruple of scalars (norm = 1)."""
        k = numpy.array([[k1, k2, k3, k4]], dtype=numpy.float64)
        return numpy.float64(self._sync(0).tri1h_quad(_lib.TRI_MOMENT["power_mmmm"], k, 0)[0])

    def i_0_4_parallelogram(self, k1, k2):
        return self._lookup("i_0_4", k1, k2)

    def i_1_1(self, k):
        """halo_trispectrum.py:625-638: _h_m(k), here from the device spline (0 outside
        [k_min, k_max])."""
        return self._lookup("i_1_1", k, k)

    def i_1_2(self, k1, k2):
        return self._lookup("i_1_2", k1, k2)

    def i_1_3(self, k1, k2, k3):
        """halo_trispectrum.py:690-705 at one triple of scalars (norm = 1)."""
        k = numpy.array([[k1, k2, k3]], dtype=numpy.float64)
        return numpy.float64(self.i_1_3_many(k)[0])

    def i_1_3_many(self, k, levels=False):
        """i_1_3 at every row of k, an (N, 3) array or a contiguous float64 torch cuda tensor."""
        k = _rows(k, 3, "triples")
        return self._sync(0, defer_status=_lib._is_torch(k)).tri_triple(k, 0, levels=levels)

    def i_1_3_parallelogram(self, k1, k2):
        return self._lookup("i_1_3", k1, k2)

    def i_2_1(self, k):
        return self._lookup("i_2_1", k, k)

    def i_2_2(self, k1, k2):
        return self._lookup("i_2_2", k1, k2)
