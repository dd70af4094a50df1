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
local_hod throughout.  HaloTrispectrum (the two- to four-halo terms) is not built.
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


class HaloTrispectrum(halo.Halo):
    """The two- to four-halo terms (halo_trispectrum.py:153-): not built."""

    def __init__(self, *args, **kws):
        raise _lib.ChompScopeError(
            "HaloTrispectrum (the two- to four-halo trispectrum terms) is outside the "
            "accelerated scope; HaloTrispectrumOneHalo is built")
