"""covariance.Covariance and CovarianceMulti for the Gaussian, super-sample and one-halo
trispectrum parts of the w(theta) covariance (covariance.py:23-871, 1085-1103), the consumer of
P(k) and the windows that SURVEY.md 8(f) ranks fourth; and covariance.CovarianceFourier, the
Gaussian covariance of C_l (covariance.py:874-1083).

Accelerated: ``Covariance(corr, corr, nongaussian_cov=False)`` -- the use of
examples/example_covariance_script.py: the projected spectrum over ln K
(``_initialize_halo_splines``), ``covariance_G`` for every pair of bins in one launch,
the Poisson term, ``get_covariance`` and ``write`` -- and with ``ssc_cov=True`` the
super-sample term on HaloSuperSampleCovariance copies of the halo:
``KernelCovariance.kernel_ssc`` (kernel.py:961-972, 1113-1231) and ``covariance_ssc`` for every
pair of bins in one call.  With ``nongaussian_cov=True`` and a
``halo_trispectrum.HaloTrispectrumOneHalo`` handed in as ``input_halo_trispectrum`` the
one-halo trispectrum term: ``KernelCovariance.kernel_NG`` (kernel.py:996-1073, 1103-1111) and
``covariance_NG`` (covariance.py:593-683) for every pair of bins in one call.  The object has
to be given: the reference never moves its default HaloTrispectrumOneHalo() off z = 0 (the
set_redshift(z_bar_NG) lines are commented out), so the redshift, the HOD and power_spec of the
trispectrum are the caller's choice.

``Covariance(corr_a, corr_b, nongaussian_cov=False)`` with two different correlations is the
Gaussian cross-covariance of two measurements (the matching_corrs == False branch,
covariance.py:422-453, 495-541): four projected spectra a, b, ab, ba on one ln K grid and
``covariance_G`` with two two-point terms, all pairs of bins in one launch; no Poisson term on the
diagonal (:312).  The reference's constructor cannot get there as shipped -- it compares the two
correlations with Correlation.__eq__ (correlation.py:119-131), which raises ValueError on the
numpy arrays in their dictionaries -- but with that one comparison answered (two objects: not
equal) the branch runs, and that is what is reproduced.  ``CovarianceMulti`` (covariance.py:796-871)
assembles the joint matrix of several correlations from such blocks.

``Covariance(corr_a, corr_b, cross_terms=True)`` adds the trispectrum and super-sample terms of
such a cross block (``nongaussian_cov=True`` with a HaloTrispectrumOneHalo, ``ssc_cov=True``):
``KernelCovariance(..., four_windows=True)`` is the reference's kernel with a1 != b1 or a2 != b2
(kernel.py:893-972, 1035-1111, 1155-1206) -- the common range of the four windows, z_bar_NG of
a1 a2 b1 b2 D^4 / chi^2, kernel_ssc and kernel_NG -- and ``covariance_ssc`` takes halo_a's response
at k_a and halo_b's at k_b (covariance.py:763-776), each halo a HaloSuperSampleCovariance copy
at its own correlation's z_bar.  The order of the two angles matters there.  Both are opt-in:
without the keyword a cross block refuses the two terms as before.  ``CovarianceMulti`` forwards
``cross_terms`` and ``ssc_cov`` to every block.

Outside the scope (ChompScopeError): ``nongaussian_cov=True`` without a HaloTrispectrumOneHalo,
the full ``HaloTrispectrum``, the trispectrum and super-sample terms of a cross block without
``cross_terms=True``, and four windows with no redshift in common.

``CovarianceFourier(l_min, l_max, KernelCovariance(...), Halo(...))`` (covariance.py:874-1083) is the
Gaussian covariance of C_l: z_bar of the four window pairs, four P_mm epochs in the halo's
context, the four Limber tables over ln l (4 x corr_npoints Romberg integrals in one launch),
their splines, and ``covariance_G(l)`` element-wise on the device.
"""
import numpy
from scipy import special

from . import _lib
from . import defaults
from . import halo as halo_mod
from . import halo_trispectrum
from . import kernel as kernel_mod
from .correlation import _POWER

deg_to_rad = numpy.pi / 180.0
rad_to_deg = 180.0 / numpy.pi
deg2_to_strad = deg_to_rad * deg_to_rad
strad_to_deg2 = rad_to_deg * rad_to_deg


class AnnulusBin(object):
    """covariance.py:1085-1103."""

    def __init__(self, inner, outer):
        self.inner = inner
        self.outer = outer
        self.center = numpy.power(10.0, 0.5 * (numpy.log10(inner) + numpy.log10(outer)))
        self.delta = outer - inner


class KernelCovariance(object):
    """kernel.KernelCovariance (kernel.py:864-1231): the four windows, the MultiEpoch, the
    common redshift / distance range, the super-sample kernel ``kernel_ssc`` and, with
    ``trispectrum_kernel=True``, the trispectrum kernel (kernel / kernel_NG / raw_kernel /
    raw_kernel_NG); without it those four raise ChompScopeError.

    Both kernels are built for a1 = b1 and a2 = b2 -- what Covariance(corr, corr) hands over --
    on the device context of ``_ssc_context`` (Covariance points it at its halo copy's, so
    the response and the table meet there) or else on a context of its own.

    With ``four_windows=True`` (a1, a2) and (b1, b2) may be different window objects
    (kernel.py:910-972): the two pairs are staged as the two slots of a cross block -- by the
    Covariance that owns this object (``_stage``), or else from two Kernels of its own -- and the
    same tables are built from the product a1 a2 b1 b2 over the range the four windows share.
    Windows with no redshift in common raise ChompScopeError.  Without the keyword four different
    windows are refused as before."""

    def __init__(self, ktheta_min, ktheta_max, window_function_a1, window_function_a2,
                 window_function_b1, window_function_b2, cosmo_multi_epoch,
                 force_quad=False, trispectrum_kernel=False, four_windows=False):
        if force_quad:
            raise _lib.ChompScopeError("force_quad=True is outside the accelerated scope")
        self.ln_ktheta_min = numpy.log(ktheta_min)
        self.ln_ktheta_max = numpy.log(ktheta_max)
        self.window_function_a1 = window_function_a1
        self.window_function_a2 = window_function_a2
        self.window_function_b1 = window_function_b1
        self.window_function_b2 = window_function_b2
        ws = (window_function_a1, window_function_a2, window_function_b1, window_function_b2)
        self.z_min = numpy.max([w.z_min for w in ws])
        self.z_max = numpy.min([w.z_max for w in ws])
        self.cosmo = cosmo_multi_epoch
        npts = defaults.default_precision["kernel_npoints"]
        self._ln_ktheta_array = numpy.linspace(self.ln_ktheta_min, self.ln_ktheta_max, npts)
        bessel = defaults.default_precision["kernel_bessel_limit"]
        self._j0_limit = special.jn_zeros(0, bessel)[-1]
        self._j0_ssc_limit = special.jn_zeros(0, int(bessel * 8))[-1]        # kernel.py:949-952
        self._j1_limit = special.jn_zeros(1, bessel)[-1]
        self._proj_kernel = None     # the Kernel whose projection tables carry the windows
        self._ssc_context = None     # callable -> device context of the table
        self._ssc_key = None
        self._ssc_table = False
        self._trispectrum_kernel = bool(trispectrum_kernel)
        self._ng_key = None
        self._ng_table = False
        self._four_windows = bool(four_windows)
        self._stage = None           # callable -> (context holding the two slots, their stamp)
        self._side_kernels = None    # without one: two Kernels of this object's own (_stage_own)
        self._own_stamp = None

    def _matching(self):
        return (self.window_function_a1 is self.window_function_b1 and
                self.window_function_a2 is self.window_function_b2)

    def _stage_own(self):
        """The two slots from two Kernels of this object's own, (a1, a2) and (b1, b2), windows
        only; in (a1, a2)'s context."""
        if self._side_kernels is None:
            kt = (numpy.exp(self.ln_ktheta_min), numpy.exp(self.ln_ktheta_max))
            self._side_kernels = (
                kernel_mod.Kernel(kt[0], kt[1], self.window_function_a1, self.window_function_a2,
                                  self.cosmo),
                kernel_mod.Kernel(kt[0], kt[1], self.window_function_b1, self.window_function_b2,
                                  self.cosmo))
        ka, kb = self._side_kernels
        ctx = ka._dev()
        stamp = (ka._signature(), kb._signature())
        if getattr(ctx, "_cov_cross_owner", None) is not self or self._own_stamp != stamp:
            ctx.covariance_cross_stage(0, ctx, _lib.CROSS_WINDOWS)
            ctx.covariance_cross_stage(1, kb._dev(), _lib.CROSS_WINDOWS)
            ctx._cov_cross_owner = self
            self._own_stamp = stamp
        return ctx, stamp

    def get_cosmology(self):
        return self.cosmo.get_cosmology()

    # -- the trispectrum kernel -------------------------------------------------------
    def _ng(self, table=True):
        """The device state of kernel_NG, on top of kernel_ssc's scalars (z_bar_NG is found
        once, there): (re)built when those were, and with `table` the 1275 integrals, their
        minimum and the bicubic of log(table - 10 min) (built only once something asks)."""
        if not self._trispectrum_kernel:
            raise _lib.ChompScopeError(
                "KernelCovariance.kernel / kernel_NG / raw_kernel / raw_kernel_NG "
                "(kernel.py:996-1073) serve the trispectrum term: pass trispectrum_kernel=True "
                "(Covariance does, given nongaussian_cov=True and a HaloTrispectrumOneHalo)")
        ctx = self._ssc(table=False)
        fresh = self._ssc_key == self._ng_key and ctx._proj_ng is self
        if not fresh or (table and not self._ng_table):
            d = self.__dict__
            d["_ng_array"], d["_ng_levels"], d["_ng_min"] = ctx.kernel_ng_setup(
                self._j0_limit, with_table=table)
            self._ng_key = self._ssc_key
            self._ng_table = table
            ctx._proj_ng = self
            if table:
                ctx.warn_cov_ng_divmax("raw_kernel_NG")
        return ctx

    def _ng_value(name):
        def get(self):
            self._ng()
            return self.__dict__["_ng_" + name]
        return property(get)

    _kernel_array = _ng_value("array")
    _kernel_levels = _ng_value("levels")
    _kernel_NG_min = _ng_value("min")
    del _ng_value

    def raw_kernel_NG(self, ln_ktheta_a, ln_ktheta_b):
        """kernel.py:1035-1073, quirk included: the norm takes ln(k theta_a) for k theta_a."""
        ctx = self._ng(table=False)
        a, b = numpy.broadcast_arrays(numpy.asarray(ln_ktheta_a, dtype=numpy.float64),
                                      numpy.asarray(ln_ktheta_b, dtype=numpy.float64))
        out = ctx.kernel_ng_raw(a.ravel(), b.ravel())
        return float(out[0]) if a.ndim == 0 else out.reshape(a.shape)

    def raw_kernel(self, ln_ktheta_a, ln_ktheta_b):
        return self.raw_kernel_NG(ln_ktheta_a, ln_ktheta_b)

    def kernel_NG(self, ln_ktheta_a, ln_ktheta_b):
        """kernel.py:999-1014: exp(spline) + 10 min on RectBivariateSpline's grid,
        [len a, len b] (callers index [0]); ln(k theta) < min is clamped to min, above max
        gives 0."""
        ctx = self._ng()
        a = numpy.asarray(ln_ktheta_a, dtype=numpy.float64)
        b = numpy.asarray(ln_ktheta_b, dtype=numpy.float64)
        a = numpy.where(a < self.ln_ktheta_min, self.ln_ktheta_min, a)
        b = numpy.where(b < self.ln_ktheta_min, self.ln_ktheta_min, b)
        inside = numpy.logical_and(a <= self.ln_ktheta_max, b <= self.ln_ktheta_max)
        ga, gb = numpy.meshgrid(numpy.atleast_1d(a).ravel(), numpy.atleast_1d(b).ravel(),
                                indexing="ij")
        grid = ctx.kernel_ng_eval(ga.ravel(), gb.ravel()).reshape(ga.shape)
        return numpy.where(inside, grid, 0.0)

    def kernel(self, ln_ktheta_a, ln_ktheta_b):
        return self.kernel_NG(ln_ktheta_a, ln_ktheta_b)

    # -- the super-sample kernel ------------------------------------------------------
    def _ssc(self, table=True):
        """The device state of kernel_ssc, (re)built when the windows, the cosmology or the
        context changed: z_bar_NG and the sigma^2 knots, and with `table` the 1275 integrals
        and the bicubic (built only once something asks for them)."""
        if self._four_windows:
            return self._ssc_four(table)
        if not self._matching():
            raise _lib.ChompScopeError(
                "kernel_ssc is accelerated for a1 = b1 and a2 = b2 (Covariance(corr, corr)); "
                "four different windows need four_windows=True (Covariance(corr_a, corr_b, "
                "cross_terms=True) passes it)")
        kern = self._proj_kernel
        if kern is None:
            kern = self._proj_kernel = kernel_mod.Kernel(
                numpy.exp(self.ln_ktheta_min), numpy.exp(self.ln_ktheta_max),
                self.window_function_a1, self.window_function_a2, self.cosmo)
        ctx = self._ssc_context() if self._ssc_context is not None else kern._dev()
        kern._setup_on(ctx)
        key = (id(ctx), kern._signature(), self.ln_ktheta_min, self.ln_ktheta_max,
               ctx.config.kernel_npoints)
        fresh = key == self._ssc_key and ctx._proj_ssc is self
        if not fresh or (table and not self._ssc_table):
            info = ctx.kernel_info()
            d = self.__dict__
            d["_ssc_chi_min"], d["_ssc_chi_max"] = float(info["chi_min"]), float(info["chi_max"])
            # kernel.py:1208-1222: sigma_r(chi, 0.0)^2 on logspace(chi_min, chi_max)
            chi = numpy.logspace(numpy.log10(d["_ssc_chi_min"]), numpy.log10(d["_ssc_chi_max"]),
                                 defaults.default_precision["corr_npoints"])
            sigma = self.cosmo.sigma_r(chi, 0.0)
            d["_ssc_ln_chi"] = numpy.log(chi)
            d["_ssc_sigma2"] = sigma * sigma
            out, d["_ssc_array"], d["_ssc_levels"] = ctx.kernel_ssc_setup(
                self.ln_ktheta_min, self.ln_ktheta_max, self._j0_ssc_limit,
                d["_ssc_ln_chi"], d["_ssc_sigma2"], with_table=table)
            d["_ssc_z_bar_NG"], _, d["_ssc_D_z_NG"] = (float(v) for v in out)
            self._ssc_key = key
            self._ssc_table = table
            ctx._proj_ssc = self
        return ctx

    def _ssc_four(self, table):
        """_ssc for four different windows: the same state, from the two staged slots."""
        if not self.z_min < self.z_max:
            raise _lib.ChompScopeError(
                "KernelCovariance: the four windows have no redshift in common (z_min = %g >= "
                "z_max = %g, kernel.py:910-916)" % (self.z_min, self.z_max))
        ctx, stamp = self._stage() if self._stage is not None else self._stage_own()
        key = (id(ctx), stamp, self.ln_ktheta_min, self.ln_ktheta_max, ctx.config.kernel_npoints)
        fresh = key == self._ssc_key and ctx._proj_ssc is self
        if not fresh or (table and not self._ssc_table):
            d = self.__dict__
            _, _, d["_ssc_chi_min"], d["_ssc_chi_max"] = ctx.covariance_cross_range()
            chi = numpy.logspace(numpy.log10(d["_ssc_chi_min"]), numpy.log10(d["_ssc_chi_max"]),
                                 defaults.default_precision["corr_npoints"])
            sigma = self.cosmo.sigma_r(chi, 0.0)
            d["_ssc_ln_chi"] = numpy.log(chi)
            d["_ssc_sigma2"] = sigma * sigma
            out, d["_ssc_array"], d["_ssc_levels"] = ctx.kernel_ssc_setup(
                self.ln_ktheta_min, self.ln_ktheta_max, self._j0_ssc_limit,
                d["_ssc_ln_chi"], d["_ssc_sigma2"], with_table=table, cross=True)
            d["_ssc_z_bar_NG"], _, d["_ssc_D_z_NG"] = (float(v) for v in out)
            self._ssc_key = key
            self._ssc_table = table
            ctx._proj_ssc = self
        return ctx

    def _ssc_value(name, table=False):
        def get(self):
            self._ssc(table)
            return self.__dict__["_ssc_" + name]
        return property(get)

    # (the reference sets these at construction, kernel.py:918-932, 961-972; here they come
    #  with the first that is asked for -- the scalars without the table, kernel.py:1132-1153)
    z_bar_NG = _ssc_value("z_bar_NG")
    chi_min = _ssc_value("chi_min")
    chi_max = _ssc_value("chi_max")
    _sigma2_ln_chi = _ssc_value("ln_chi")
    _sigma2_knots = _ssc_value("sigma2")
    _D_z_NG = _ssc_value("D_z_NG")
    _kernel_ssc_array = _ssc_value("array", True)
    _kernel_ssc_levels = _ssc_value("levels", True)
    del _ssc_value

    def _sigma2(self, chi):
        """kernel.py:1224-1231."""
        ctx = self._ssc(table=False)
        c = numpy.asarray(chi, dtype=numpy.float64)
        with numpy.errstate(invalid="ignore", divide="ignore"):
            s = ctx.spline_eval(self._sigma2_ln_chi, self._sigma2_knots,
                                numpy.log(numpy.atleast_1d(c)).ravel())
        out = numpy.where((c.ravel() >= self.chi_min) & (c.ravel() <= self.chi_max), s, 0.0)
        return out.reshape(c.shape)

    def raw_kernel_ssc(self, ln_ktheta_a, ln_ktheta_b):
        """kernel.py:1155-1206, quirks included: the Romberg over [ln chi_min, ln chi_max']
        hands ln chi to the integrand as chi, and the norm takes ln(k theta_a) for k theta_a."""
        ctx = self._ssc(table=False)
        a, b = numpy.broadcast_arrays(numpy.asarray(ln_ktheta_a, dtype=numpy.float64),
                                      numpy.asarray(ln_ktheta_b, dtype=numpy.float64))
        out = ctx.kernel_ssc_raw(a.ravel(), b.ravel())
        return float(out[0]) if a.ndim == 0 else out.reshape(a.shape)

    def kernel_ssc(self, ln_ktheta_a, ln_ktheta_b):
        """kernel.py:1113-1130: RectBivariateSpline's grid-shaped result, [len a, len b]
        (callers index [0]); ln(k theta) <= min is clamped to min, above max gives 0."""
        ctx = self._ssc()
        a = numpy.asarray(ln_ktheta_a, dtype=numpy.float64)
        b = numpy.asarray(ln_ktheta_b, dtype=numpy.float64)
        a = numpy.where(a <= self.ln_ktheta_min, self.ln_ktheta_min, a)
        b = numpy.where(b <= self.ln_ktheta_min, self.ln_ktheta_min, b)
        inside = numpy.logical_and(a <= self.ln_ktheta_max, b <= self.ln_ktheta_max)
        ga, gb = numpy.meshgrid(numpy.atleast_1d(a).ravel(), numpy.atleast_1d(b).ravel(),
                                indexing="ij")
        grid = ctx.kernel_ssc_eval(ga.ravel(), gb.ravel()).reshape(ga.shape)
        return numpy.where(inside, grid, 0.0)


class Covariance(object):
    """covariance.py:23-200."""

    def __init__(self, input_correlation_a, input_correlation_b,
                 bins_per_decade=5.0, survey_area_deg2=20,
                 n_a=1.0e4, n_b=1.0e4, variance=1.0, nongaussian_cov=True,
                 input_halo_trispectrum=None, power_spec='power_mm',
                 poisson_noise_only=False, ssc_cov=False, cross_terms=False, **kws):
        cross = input_correlation_a is not input_correlation_b
        if cross:
            self._check_cross(input_correlation_a, input_correlation_b, nongaussian_cov, ssc_cov,
                              cross_terms)
        if nongaussian_cov and input_halo_trispectrum is None:
            raise _lib.ChompScopeError(
                "the trispectrum term of the covariance (covariance_NG) is built for an explicit "
                "one-halo trispectrum: pass input_halo_trispectrum=halo_trispectrum."
                "HaloTrispectrumOneHalo(redshift, ...) -- the reference's default object stays "
                "at z = 0 whatever z_bar_NG is -- or nongaussian_cov=False")
        if not nongaussian_cov and input_halo_trispectrum is not None:
            raise _lib.ChompScopeError(
                "input_halo_trispectrum with nongaussian_cov=False: the trispectrum term "
                "(covariance_NG) would not be used; pass nongaussian_cov=True to build it")
        if nongaussian_cov and not isinstance(input_halo_trispectrum,
                                              halo_trispectrum.HaloTrispectrumOneHalo):
            raise _lib.ChompScopeError(
                "the trispectrum term of the covariance is accelerated for a halo_trispectrum."
                "HaloTrispectrumOneHalo, not %s (HaloTrispectrum, the two- to four-halo terms, "
                "is outside the scope)" % type(input_halo_trispectrum).__name__)
        self.annular_bins = []
        self.log_theta_min = input_correlation_a.log_theta_min
        self.log_theta_max = input_correlation_a.log_theta_max
        unit_double = numpy.floor(self.log_theta_min) * bins_per_decade
        theta = numpy.power(10.0, unit_double / (1.0 * bins_per_decade))
        self.bins_per_decade = bins_per_decade
        self.corr_a = input_correlation_a
        self.corr_b = input_correlation_b
        # covariance.py:61-64.  Correlation.__eq__ (correlation.py:119-131) compares attribute
        # dictionaries -- numpy arrays included -- and raises "ValueError: The truth value of an
        # array ... is ambiguous" for two different objects; it can return True only for one
        # object given twice.  For two objects the answer it could not give is False.
        self.matching_corrs = not cross
        while theta < numpy.power(10.0, self.log_theta_max):
            if (theta >= numpy.power(10.0, self.log_theta_min) and
                    theta < numpy.power(10.0, self.log_theta_max)):
                self.annular_bins.append(AnnulusBin(
                    theta, numpy.power(10.0, (unit_double + 1.0) / (1.0 * bins_per_decade))))
            unit_double += 1.0
            theta = numpy.power(10.0, unit_double / (1.0 * bins_per_decade))

        self.area = survey_area_deg2 * deg2_to_strad
        try:
            self.n_a1, self.n_a2 = n_a[0], n_a[1]
        except (TypeError, IndexError):
            self.n_a1 = self.n_a2 = n_a
        try:
            self.n_b1, self.n_b2 = n_b[0], n_b[1]
        except (TypeError, IndexError):
            self.n_b1 = self.n_b2 = n_b
        self.nongaussian_cov = bool(nongaussian_cov)
        self.halo_tri = input_halo_trispectrum
        self.ssc_cov = bool(ssc_cov)
        self.poisson_noise_only = poisson_noise_only

        kern = input_correlation_a.kernel
        kern_b = input_correlation_b.kernel
        self.kernel = KernelCovariance(
            numpy.power(10.0, self.log_theta_min) * defaults.default_limits["k_min"],
            numpy.power(10.0, self.log_theta_max) * defaults.default_limits["k_max"],
            kern.window_function_a, kern.window_function_b,
            kern_b.window_function_a, kern_b.window_function_b, kern.cosmo,
            trispectrum_kernel=self.nongaussian_cov, four_windows=cross and bool(cross_terms))
        # covariance.py:108-115.  The reference's Kernel holds *copies* of its two
        # windows, each with a private copy of the MultiEpoch, and WindowFunction.__eq__
        # (kernel.py:248-259) compares those by identity: two windows are "equal" only
        # when they are the same object.  With one correlation given twice that is the
        # case for the pairs (a1, b1) and (a2, b2) and for no other, whatever the windows.
        # Two correlations hold those same objects only when they share their Kernel: the
        # windows of two Kernels are different copies even when made from one window.
        same = kern is kern_b
        self.equal_windows = [False, False, False, False, same, same]
        self.density = [self.n_a1 / self.area, self.n_a2 / self.area,
                        self.n_b1 / self.area, self.n_b2 / self.area,
                        self.n_a1 / self.area, self.n_a2 / self.area]
        self.variance = variance
        self.cosmic_shear = self._identify_cosmic_shear()

        # covariance.py:144-151: with ssc_cov the halo objects are HaloSuperSampleCovariance
        # copies made now, with whatever tables the correlation's halo has built by now; the
        # Gaussian term is then projected from halo_a, not from the correlation's halo
        if self.ssc_cov:
            self.halo_a = halo_mod.HaloSuperSampleCovariance.init_from_halo(
                input_correlation_a.halo)
            self.halo_b = halo_mod.HaloSuperSampleCovariance.init_from_halo(
                input_correlation_b.halo)
        else:
            self.halo_a = input_correlation_a.halo
            self.halo_b = input_correlation_b.halo
        # kernel_ssc and kernel_NG live in halo_a's context (the first beside the response it is
        # integrated with)
        self.kernel._proj_kernel = kern
        self.kernel._ssc_context = lambda: self.halo_a._context()
        # ... and of a cross block from the two slots its Gaussian tables are built from
        self.kernel._stage = lambda: (self._table_cross(), self._cross_stamp)
        self._cross_stamp = 0
        self._copy_keys = None
        self._initialized_halo_splines = False
        self._table_key = None
        self._ln_k_min = numpy.log(defaults.default_limits['k_min'])
        self._ln_k_max = numpy.log(defaults.default_limits['k_max'])
        self._j0_limit = special.jn_zeros(
            0, defaults.default_precision["kernel_bessel_limit"])[-1]
        if power_spec is None:
            power_spec = 'linear_power'
        if (power_spec not in _POWER or not hasattr(self.halo_a, power_spec) or
                not hasattr(self.halo_b, power_spec)):
            print("WARNING: Invalid input for power spectra variable,")
            print("\t setting to linear_power")
            power_spec = 'linear_power'
        self.power_spec = power_spec

    @staticmethod
    def _check_cross(corr_a, corr_b, nongaussian_cov, ssc_cov, cross_terms=False):
        """The limits of a cross block, Covariance(corr_a, corr_b) of two different objects."""
        if (nongaussian_cov or ssc_cov) and not cross_terms:
            raise _lib.ChompScopeError(
                "Covariance of two different correlation objects is accelerated for its Gaussian "
                "term only: the trispectrum and super-sample terms of a cross block are outside "
                "the scope -- pass nongaussian_cov=False (and leave ssc_cov=False), or opt in to "
                "both terms with cross_terms=True")
        for corr in (corr_a, corr_b):
            if not isinstance(corr.halo, halo_mod.Halo):
                # (the two sides are staged from their halos' device contexts)
                raise _lib.ChompScopeError(
                    "Covariance of two different correlation objects needs a chomp_amd halo.Halo "
                    "(or a subclass) behind each of them, not %s" % type(corr.halo).__name__)
        cos_a, cos_b = corr_a.kernel.cosmo, corr_b.kernel.cosmo
        if sorted(cos_a.cosmo_dict.items()) != sorted(cos_b.cosmo_dict.items()):
            raise _lib.ChompScopeError(
                "Covariance of two correlations whose MultiEpoch cosmologies differ: distances "
                "and growth are taken from correlation a's alone (covariance.py:93-102), which "
                "has no meaning for b's windows; give both one cosmology")
        names = [getattr(c, "_power_name", None) for c in (corr_a, corr_b)]
        if None not in names and names[0] != names[1]:
            raise _lib.ChompScopeError(
                "Covariance of two correlations with different power_spec (%s, %s): one "
                "spectrum name serves both halos (covariance.py:551-586)" % tuple(names))

    def _identify_cosmic_shear(self):
        shear = [isinstance(w, kernel_mod.WindowFunctionConvergence) for w in (
            self.kernel.window_function_a1, self.kernel.window_function_a2,
            self.kernel.window_function_b1, self.kernel.window_function_b2)]
        return [shear[0] * shear[1] or shear[2] * shear[3],
                shear[0] * shear[3] or shear[1] * shear[2]]

    # -- device tables -----------------------------------------------------------
    def _prepare_copy(self):
        """Correlation._prepare on halo_a (ssc_cov): the windows' tables go into the copy's
        context, and the copy is moved to z_bar as _initialize_halo_splines does (:460-461)."""
        z_bar = self.corr_a.kernel.z_bar
        self.halo_a.set_redshift(z_bar)
        self.halo_b.set_redshift(z_bar)
        code, need = _POWER[self.power_spec]
        self.corr_a.kernel._setup_on(self.halo_a._context())
        return self.halo_a._sync(need), self.halo_a._power_code(code)

    def _table(self):
        """Projected spectrum over ln K in the device context of the correlation, or of
        halo_a with ssc_cov (covariance.py:455-543); rebuilt when anything it was built from
        has changed."""
        if self.ssc_cov:
            ctx, code = self._prepare_copy()
        else:
            ctx, code = self.corr_a._prepare(self.power_spec)
        h = self.halo_a
        hod = h.get_hod_object()
        key = (id(ctx), self.corr_a.kernel._signature(), code, h._epoch_sig, h._mass_sig,
               type(hod), tuple(getattr(hod, a, None) for a in ("log_M_min", "sigma", "log_M_0",
                                                                "log_M_1p", "alpha", "w")),
               repr(sorted(h._profile_dict.items())), h.get_extrapolation(),
               self.corr_a.kernel.z_bar)
        if key != self._table_key or not self._initialized_halo_splines:
            self._z_bar_G_a = self._z_bar_G_b = self.corr_a.kernel.z_bar
            self._D_z_a = self._D_z_b = self.corr_a._growth_at_z_bar()
            self._ln_K_array, self._halo_a_array, self._halo_a_levels = \
                ctx.covariance_table(code, 0, self._D_z_a)
            self._ln_K_min, self._ln_K_max = self._ln_K_array[0], self._ln_K_array[-1]
            self._table_key = key
            self._initialized_halo_splines = True
        return ctx

    @staticmethod
    def _halo_signature(h):
        """Everything a halo's spectrum is built from, readable without the device."""
        hod = h.get_hod_object()
        return (id(h), type(h).__name__, tuple(sorted(h.cosmo.cosmo_dict.items())),
                h.cosmo._redshift, bool(getattr(h.cosmo, "_with_bao", False)),
                tuple(sorted(h.mass.halo_dict.items())), h.mass._kind, type(hod),
                tuple(getattr(hod, a, None) for a in ("log_M_min", "sigma", "log_M_0",
                                                      "log_M_1p", "alpha", "w")),
                repr(sorted(h._profile_dict.items())), h.get_extrapolation())

    def _table_cross(self):
        """The four projected spectra a, b, ab, ba of a cross block over one ln K grid
        (covariance.py:455-543, matching_corrs == False), in the device context of correlation
        a's halo; rebuilt when anything they were built from has changed.

        Each side is set up where it lives -- its Kernel and its halo at its own z_bar, in its
        halo's context -- and a snapshot of it is staged into a's context, so neither two
        Halo objects nor one shared by both correlations have to hold two set-ups at once.  When
        ``corr_a.halo is corr_b.halo`` the reference's two set_redshift calls (:465-466) leave
        that one object at z_bar_b: both spectra are then P at z_bar_b, here as there."""
        ca, cb = self.corr_a, self.corr_b
        z_a, z_b = ca.kernel.z_bar, cb.kernel.z_bar
        if self.ssc_cov:
            self._renew_copies(z_a, z_b)
        ha, hb = self.halo_a, self.halo_b
        if ha is not hb:
            ha.set_redshift(z_a)
        hb.set_redshift(z_b)
        ctx = ha._context()
        key = (id(ctx), self.power_spec, ca.kernel._signature(), cb.kernel._signature(),
               z_a, z_b, self._halo_signature(ha), self._halo_signature(hb))
        if (key != self._table_key or not self._initialized_halo_splines or
                getattr(ctx, "_cov_cross_owner", None) is not self):
            self._z_bar_G_a, self._z_bar_G_b = z_a, z_b
            # covariance.py:468-469: both from correlation a's MultiEpoch
            self._D_z_a = ca._growth_at_z_bar()
            self._D_z_b = float(ca.kernel.cosmo.growth_factor(z_b))
            ctx_a, code_a = self._prepare_side(ca, ha)
            ctx.covariance_cross_stage(0, ctx_a, code_a)
            ctx_b, code_b = self._prepare_side(cb, hb)
            ctx.covariance_cross_stage(1, ctx_b, code_b)
            self._cross_stamp += 1     # (what was built from the slots -- kernel_ssc, kernel_NG -- is void)
            self._ln_K_array, tab, lev = ctx.covariance_table_cross(self._D_z_a, self._D_z_b)
            (self._halo_a_array, self._halo_b_array, self._halo_ab_array,
             self._halo_ba_array) = tab
            (self._halo_a_levels, self._halo_b_levels, self._halo_ab_levels,
             self._halo_ba_levels) = lev
            self._ln_K_min, self._ln_K_max = self._ln_K_array[0], self._ln_K_array[-1]
            self._table_key = key
            self._initialized_halo_splines = True
            ctx._cov_cross_owner = self
        return ctx

    def _prepare_side(self, corr, h):
        """One side of a cross block set up where it lives: Correlation._prepare; with ssc_cov on
        the halo copy instead (as _prepare_copy), whose epoch then also holds the tables of the
        response; so does that of a HaloSuperSampleCovariance handed in by the caller."""
        if hasattr(h, "dln_power_ddelta_b"):
            h._sync(_lib.FAM_SSC)
        if not self.ssc_cov:
            return corr._prepare(self.power_spec)
        code, need = _POWER[self.power_spec]
        corr.kernel._setup_on(h._context())
        return h._sync(need | _lib.FAM_SSC), h._power_code(code)

    def _renew_copies(self, z_a, z_b):
        """The HaloSuperSampleCovariance copies of a cross block follow their correlations: the
        reference makes them once, at construction (covariance.py:144-149), and a copy keeps the
        I_1^2 knots of its first build whatever is set on it later; after a change of a
        correlation's windows, z_bar, HOD or halo the side's copy is made again, so the block
        holds what one built from the changed correlations would."""
        keys = [(c.kernel._signature(), z, self._halo_signature(c.halo))
                for c, z in ((self.corr_a, z_a), (self.corr_b, z_b))]
        if self._copy_keys is not None:
            if keys[0] != self._copy_keys[0]:
                self.halo_a = halo_mod.HaloSuperSampleCovariance.init_from_halo(self.corr_a.halo)
            if keys[1] != self._copy_keys[1]:
                self.halo_b = halo_mod.HaloSuperSampleCovariance.init_from_halo(self.corr_b.halo)
        self._copy_keys = keys

    def _tables(self):
        return self._table() if self.matching_corrs else self._table_cross()

    def _initialize_halo_splines(self):
        self._initialized_halo_splines = False
        self._tables()

    def _projected(self, name, K):
        ctx = self._tables()
        return ctx.spline_eval(self._ln_K_array, getattr(self, "_halo_%s_array" % name),
                               numpy.log(K))

    def _projected_halo_a(self, K):
        return self._projected("a", K)

    def _projected_halo_b(self, K):
        """covariance.py:215-224: a's spline for one correlation given twice."""
        return self._projected("a" if self.matching_corrs else "b", K)

    def _projected_halo_ab(self, K):
        return self._projected("ab", K)

    def _projected_halo_ba(self, K):
        return self._projected("ba", K)

    def set_cosmology(self, cosmo_dict):
        if not self.matching_corrs:
            # (the reference would go on with the KernelCovariance, its chi limits and the
            #  halo objects of the old cosmology in part: covariance.py:252-270)
            raise _lib.ChompScopeError(
                "Covariance.set_cosmology on a cross covariance (two different correlation "
                "objects) is outside the scope: set the cosmology of both correlations and "
                "build a new Covariance")
        if self.ssc_cov:
            # The reference ends in AttributeError here whatever ssc_cov is
            # (HaloTrispectrumOneHalo.set_cosmology dereferences pert=None); with ssc_cov it
            # would also have left halo_a the plain halo and kept the old kernel_ssc spline.
            raise _lib.ChompScopeError(
                "Covariance.set_cosmology with ssc_cov=True: the reference raises "
                "AttributeError (covariance.py:262-270, halo_trispectrum.py) and would keep the "
                "HaloSuperSampleCovariance copies and the kernel_ssc spline of the old cosmology; "
                "build a new Covariance instead")
        self.corr_a.set_cosmology(cosmo_dict)
        self.halo_a = self.halo_b = self.corr_a.halo
        self._initialized_halo_splines = False
        if self.nongaussian_cov:
            # covariance.py:268: the trispectrum moves to z_bar_NG of the new cosmology -- the
            # kernel state is rebuilt for it first (its key holds the cosmology).  With
            # pert=None this raises AttributeError after the halo model has moved, as the
            # reference does; covariance_NG reads the object's table anew at every call.
            self.halo_tri.set_cosmology(cosmo_dict, self.kernel.z_bar_NG)

    def get_cosmology(self):
        return self.kernel.get_cosmology()

    # -- covariance --------------------------------------------------------------
    @property
    def D_z_NG(self):
        """covariance.py:143: MultiEpoch.growth_factor(z_bar_NG)."""
        self.kernel._ssc(table=False)
        return self.kernel._D_z_NG

    def get_covariance(self):
        """covariance.py:297-317; the Gaussian term of all bin pairs is one launch, the
        trispectrum and super-sample terms one call each."""
        nb = len(self.annular_bins)
        iu = numpy.triu_indices(nb)
        centers = numpy.array([b.center for b in self.annular_bins])
        vals = None
        if not self.poisson_noise_only and nb:
            vals = self._covariance_G_pairs(centers[iu[0]], centers[iu[1]])
            if self.nongaussian_cov:
                vals = vals + self._covariance_NG_pairs(centers[iu[0]], centers[iu[1]])
            if self.ssc_cov:
                vals = vals + self._covariance_ssc_pairs(centers[iu[0]], centers[iu[1]])
        return self._fill_covar(vals)

    def _fill_covar(self, vals):
        """`covar` from the values of the bin pairs (a, b), a <= b, in numpy.triu_indices order
        (None: no such term), and the Poisson diagonal of a matching block."""
        nb = len(self.annular_bins)
        self.covar = numpy.zeros((nb, nb))
        if vals is not None:
            iu = numpy.triu_indices(nb)
            self.covar[iu] = vals
            self.covar[(iu[1], iu[0])] = vals
        if self.matching_corrs:                              # covariance.py:312
            for i, b in enumerate(self.annular_bins):
                self.covar[i, i] += self.covariance_P(b.delta, b.center)
        return self.covar

    def covariance(self, annular_bin_a, annular_bin_b):
        """covariance.py:319-351."""
        cov_P = 0.0
        if annular_bin_a is annular_bin_b and self.matching_corrs:
            cov_P = self.covariance_P(annular_bin_a.delta, annular_bin_a.center)
        if self.poisson_noise_only:
            return cov_P
        res = self.covariance_G(annular_bin_a.center, annular_bin_b.center,
                                annular_bin_a.delta, annular_bin_b.delta)
        if self.nongaussian_cov:
            res += self.covariance_NG(annular_bin_a.center, annular_bin_b.center)
        if self.ssc_cov:
            res += self.covariance_ssc(annular_bin_a.center, annular_bin_b.center)
        return res + cov_P

    def covariance_P(self, delta, theta, window_1=0, window_2=1):
        """covariance.py:338-359."""
        term1 = (self.proj_power_poisson(0) * self.proj_power_poisson(2) *
                 (1. + self.cosmic_shear[0]))
        term2 = (self.proj_power_poisson(3) * self.proj_power_poisson(1) *
                 (1. + self.cosmic_shear[1]))
        term3 = (self.proj_power_poisson(4) * self.proj_power_poisson(5) *
                 (1. + self.cosmic_shear[1]))
        return (term1 + term2 + term3) / (2. * numpy.pi * self.area * theta * delta)

    def proj_power_poisson(self, window_pair=0):
        if self.equal_windows[window_pair]:
            return self.variance * self.variance / self.density[window_pair]
        return 0.0

    def _covariance_G_pairs(self, theta_a, theta_b):
        if not self.matching_corrs:
            ctx = self._table_cross()
            return ctx.covariance_gaussian_cross(
                self._j0_limit, self.area, [self.proj_power_poisson(p) for p in range(4)],
                theta_a, theta_b)
        ctx = self._table()
        return ctx.covariance_gaussian(self._j0_limit, self.area,
                                       self.proj_power_poisson(0),
                                       self.proj_power_poisson(2), theta_a, theta_b)

    def covariance_G(self, theta_a, theta_b, delta_a=None, delta_b=None):
        """covariance.py:361-395 (the bin widths do not enter the integrand as shipped)."""
        ta = numpy.asarray(theta_a, dtype=numpy.float64)
        out = self._covariance_G_pairs(ta.ravel(), numpy.asarray(theta_b,
                                                                 dtype=numpy.float64).ravel())
        return float(out[0]) if ta.ndim == 0 else out.reshape(ta.shape)

    def _covariance_NG_pairs(self, theta_a, theta_b, knots=False):
        if not self.nongaussian_cov:
            raise _lib.ChompScopeError(
                "covariance_NG needs the trispectrum term: Covariance(..., nongaussian_cov=True, "
                "input_halo_trispectrum=HaloTrispectrumOneHalo(...))")
        tri = self.halo_tri
        if not tri._initialized_i_0_4:
            tri._initialize_i_0_4()
        ctx = self.kernel._ng()
        out = ctx.covariance_ng(self.area, tri._i_0_4_array, tri._k_min, tri._k_max,
                                theta_a, theta_b, knots)
        ctx.warn_cov_ng_divmax("covariance_NG")
        return out

    def covariance_NG(self, theta_a_rad, theta_b_rad):
        """covariance.py:593-683: for each k_a knot a Romberg over ln k_b of
        k_b^2 T(k_a, k_b) kernel_NG(ln k_a theta_a, ln k_b theta_b) / D(z_bar_NG)^4, T =
        halo_tri's trispectrum_parallelogram at that object's own redshift; their spline, and
        the Romberg over ln k_a / (4 pi^2 area)."""
        ta, tb = numpy.broadcast_arrays(numpy.asarray(theta_a_rad, dtype=numpy.float64),
                                        numpy.asarray(theta_b_rad, dtype=numpy.float64))
        out = self._covariance_NG_pairs(ta.ravel(), tb.ravel())
        return float(out[0]) if ta.ndim == 0 else out.reshape(ta.shape)

    def _covariance_ssc_pairs(self, theta_a, theta_b, knots=False):
        if not hasattr(self.halo_a, "dln_power_ddelta_b"):
            # covariance.py:772: the reference's integrand asks halo_a for it
            raise AttributeError("'%s' object has no attribute 'dln_power_ddelta_b'"
                                 % type(self.halo_a).__name__)
        if not self.matching_corrs:
            if not hasattr(self.halo_b, "dln_power_ddelta_b"):
                raise AttributeError("'%s' object has no attribute 'dln_power_ddelta_b'"
                                     % type(self.halo_b).__name__)
            # (the slots hold both responses: _prepare_side)
            return self.kernel._ssc().covariance_ssc_cross(self.area, theta_a, theta_b, knots)
        ctx = self.kernel._ssc()
        self.halo_a._sync(_lib.FAM_SSC)
        return ctx.covariance_ssc(0, self.area, theta_a, theta_b, knots)

    def covariance_ssc(self, theta_a_rad, theta_b_rad):
        """covariance.py:685-776: for each k_a knot a Romberg over ln k_b of
        k_b^2 R(k_a) R(k_b) kernel_ssc(ln k_a theta_a, ln k_b theta_b), R = halo_a's
        dln_power_ddelta_b (in a cross block halo_a's at k_a and halo_b's at k_b, so the order of
        the two angles matters); their spline, and the Romberg over ln k_a / (4 pi^2 area)."""
        ta, tb = numpy.broadcast_arrays(numpy.asarray(theta_a_rad, dtype=numpy.float64),
                                        numpy.asarray(theta_b_rad, dtype=numpy.float64))
        out = self._covariance_ssc_pairs(ta.ravel(), tb.ravel())
        return float(out[0]) if ta.ndim == 0 else out.reshape(ta.shape)

    def write(self, file_name):
        """covariance.py:778-793."""
        with open(file_name, 'w') as f:
            f.write("#ttype1 = theta_a [deg]\n#ttype2 = theta_b [deg]\n" +
                    "#ttype3 = covariance\n")
            for idx_a, bin_a in enumerate(self.annular_bins):
                for idx_b, bin_b in enumerate(self.annular_bins):
                    f.writelines('%1.16f %1.16f %1.16f\n' % (
                        bin_a.center * rad_to_deg, bin_b.center * rad_to_deg,
                        self.covar[idx_a, idx_b]))


class CovarianceMulti(Covariance):
    """covariance.py:796-871: the joint covariance of several correlations, one Covariance per
    pair (i <= j) in ``covariance_list[i][j - i]``, assembled into ``wcovar`` by
    ``get_covariance``.  Every block owns its tables.  With more than one correlation the
    off-diagonal blocks are cross-covariances, Gaussian term only: pass nongaussian_cov=False
    (the default, True, is the reference's, and raises ChompScopeError for them) -- or
    cross_terms=True, which every block receives and which opens the trispectrum and super-sample
    terms of the cross blocks (Covariance).  ssc_cov is forwarded too; the reference forwards
    neither, and the defaults leave its behaviour."""

    def __init__(self, correlation_object_list, bins_per_decade=5,
                 survey_area_deg2=4 * numpy.pi * strad_to_deg2,
                 n_a=1e6, n_b=1e6, variance=1.0, nongaussian_cov=True,
                 input_halo_trispectrum=None, poisson_noise_only=False, cross_terms=False,
                 ssc_cov=False, **kws):
        self.covariance_list = []
        n = len(correlation_object_list)
        for idx1 in range(n):
            row = []
            for idx2 in range(idx1, n):
                row.append(Covariance(
                    input_correlation_a=correlation_object_list[idx1],
                    input_correlation_b=correlation_object_list[idx2],
                    bins_per_decade=bins_per_decade, survey_area_deg2=survey_area_deg2,
                    n_a=n_a, n_b=n_b, variance=variance, nongaussian_cov=nongaussian_cov,
                    input_halo_trispectrum=input_halo_trispectrum,
                    poisson_noise_only=poisson_noise_only, ssc_cov=ssc_cov,
                    cross_terms=cross_terms))
            self.covariance_list.append(row)
        self.annular_bins = self.covariance_list[0][0].annular_bins
        self.theta_bins = len(self.annular_bins)
        self.wcovar = numpy.empty((self.theta_bins * n, self.theta_bins * n))

    def get_covariance(self):
        """covariance.py:854-871: block (i, j) and its mirror both receive the block's covar."""
        for row in self.covariance_list:
            for cov in row:
                cov.get_covariance()
        return self._assemble()

    def _assemble(self):
        """wcovar from the blocks' covar (covariance.py:862-870)."""
        for idx1, row in enumerate(self.covariance_list):
            for idx2, cov in enumerate(row):
                row_ndx1 = idx1 * self.theta_bins
                row_ndx2 = row_ndx1 + self.theta_bins
                col_ndx1 = (idx1 + idx2) * self.theta_bins
                col_ndx2 = col_ndx1 + self.theta_bins
                self.wcovar[row_ndx1:row_ndx2, col_ndx1:col_ndx2] = cov.covar
                self.wcovar[col_ndx1:col_ndx2, row_ndx1:row_ndx2] = cov.covar
        return self.wcovar

    # -- every block in one call -------------------------------------------------
    def _batched_scope(self, trispectrum=False, tabulated=False):
        """ChompScopeError unless get_covariance_batched serves these blocks; no device work.
        Returns (the correlations, the spectrum's name).  trispectrum: the caller opted in to the
        one-halo trispectrum term (get_covariance_batched(trispectrum=True)); without it blocks
        built with nongaussian_cov are refused as they always were.  tabulated: the caller opted
        in to tabulated redshift distributions, refused without it as they always were."""
        from . import cosmology
        from . import hod as hod_mod

        def refuse(why):
            raise _lib.ChompScopeError("get_covariance_batched: %s; use get_covariance" % why)
        blocks = [cov for row in self.covariance_list for cov in row]
        corrs = [row[0].corr_a for row in self.covariance_list]
        if not trispectrum and any(cov.nongaussian_cov for cov in blocks):
            refuse("the batch serves the Gaussian and Poisson terms, not the trispectrum "
                   "(nongaussian_cov) or super-sample (ssc_cov) terms")
        ng = bool(blocks[0].nongaussian_cov)
        if any(bool(cov.nongaussian_cov) != ng for cov in blocks):
            refuse("the blocks differ in nongaussian_cov: the batch adds the trispectrum term to "
                   "every block or to none")
        if ng and any(cov.halo_tri is not blocks[0].halo_tri for cov in blocks):
            refuse("the blocks do not share one halo_tri object: the batch takes one I_0^4 table "
                   "for all of them")
        ssc = bool(blocks[0].ssc_cov)
        if any(bool(cov.ssc_cov) != ssc for cov in blocks):
            refuse("the blocks differ in ssc_cov: the batch adds the super-sample term to every "
                   "block or to none")
        if any(cov.poisson_noise_only for cov in blocks):
            refuse("poisson_noise_only needs no device")
        names = set(cov.power_spec for cov in blocks)
        if len(names) != 1:
            refuse("the blocks' power_spec differ (%s)" % ", ".join(sorted(names)))
        centers = [[b.center for b in cov.annular_bins] for cov in blocks]
        if any(c != centers[0] for c in centers) or any(cov.area != blocks[0].area for cov in blocks):
            refuse("the blocks' angular bins or survey areas differ")
        if ssc or ng:
            k0 = blocks[0].kernel
            # (the J0 limit of each term that is asked for: _j0_ssc_limit, _j0_limit)
            limits = [name for name, on in (("_j0_ssc_limit", ssc), ("_j0_limit", ng)) if on]

            def shared(k):
                return (k.ln_ktheta_min, k.ln_ktheta_max) + tuple(getattr(k, a) for a in limits)
            for i, row in enumerate(self.covariance_list):
                for j, cov in enumerate(row, i):
                    k = cov.kernel
                    if shared(k) != shared(k0):
                        refuse("block (%d, %d): its KernelCovariance has another k theta range "
                               "or J0 limit than that of block (0, 0)" % (i, j))
                    if not k.z_min < k.z_max:
                        refuse("block (%d, %d): the four windows have no redshift in common "
                               "(z_min = %g >= z_max = %g, kernel.py:910-916)"
                               % (i, j, k.z_min, k.z_max))
        first = corrs[0].kernel
        for i, corr in enumerate(corrs):
            k = corr.kernel
            if type(k) is not kernel_mod.Kernel:
                refuse("the kernel of correlation %d is a %s, the batch takes kernel.Kernel"
                       % (i, type(k).__name__))
            if k._z_bar_override is not None:
                refuse("the kernel of correlation %d has an assigned z_bar "
                       "(Correlation.set_redshift); the batch finds z_bar per kernel" % i)
            for name in ("window_function_a", "window_function_b"):
                dist = getattr(getattr(k, name, None), "_redshift_dist", None)
                if not tabulated and isinstance(dist, kernel_mod.dNdzInterpolation):
                    refuse("correlation %d: %s has a tabulated redshift distribution (%s)"
                           % (i, name, type(dist).__name__))
            if cosmology.has_dark_energy(k.cosmo.cosmo_dict):
                refuse("the kernel of correlation %d has a w0-wa cosmology" % i)
            if tuple(k._ktheta) != tuple(first._ktheta):
                refuse("the kernel of correlation %d has another k theta range than that of "
                       "correlation 0" % i)
            who = "get_covariance_batched"
            try:
                corr._hods_scope(who=who, loop="")
            except _lib.ChompScopeError as e:
                why = str(e)[len(who) + 2:].rsplit("; use the loop", 1)[0]
                refuse("correlation %d: %s" % (i, why))
            if type(corr.halo.local_hod) not in (hod_mod.HODZheng, hod_mod.HODMandelbaum):
                refuse("the HOD of correlation %d is a %s, not an HODZheng or HODMandelbaum"
                       % (i, type(corr.halo.local_hod).__name__))
        h0 = corrs[0].halo
        for i, corr in enumerate(corrs):
            h = corr.halo
            if (sorted(h.mass.halo_dict.items()) != sorted(h0.mass.halo_dict.items()) or
                    getattr(h.mass, "_kind", 0) != getattr(h0.mass, "_kind", 0)):
                refuse("the halo of correlation %d has another halo dictionary or mass function "
                       "than that of correlation 0 (one grid.HaloGrid takes one of each)" % i)
            for j in range(i):
                if corrs[j].halo is h:
                    refuse("correlations %d and %d share one Halo object: the loop then "
                           "evaluates both sides of their block at one redshift" % (j, i))
        for i, ca in enumerate(corrs):
            for cb in corrs[i + 1:]:
                try:
                    self._check_cross(ca, cb, False, False)
                except _lib.ChompScopeError as e:
                    refuse(str(e))
        return corrs, names.pop()

    @staticmethod
    def _ssc_blocks_knots(cosmos, ranges):
        """The sigma^2 knots of every block, (ln chi, sigma^2), each [n_blocks, corr_npoints], as
        KernelCovariance._ssc / _ssc_four lay them (kernel.py:1208-1222): block (i, j) takes
        logspace(log10 chi_min, log10 chi_max, corr_npoints) of its own range -- ranges
        [n_blocks, 4] = z_min, z_max, chi_min, chi_max, the blocks in the row-major order of the
        upper triangle -- and sigma_r(chi, 0.0)^2 of correlation i's MultiEpoch, cosmos[i]: one
        sigma_r call per row i of blocks."""
        n = len(cosmos)
        npts = defaults.default_precision["corr_npoints"]
        ranges = numpy.asarray(ranges, dtype=numpy.float64).reshape(n * (n + 1) // 2, 4)
        ln_chi = numpy.empty((ranges.shape[0], npts))
        sigma2 = numpy.empty((ranges.shape[0], npts))
        b = 0
        for i, cosmo in enumerate(cosmos):
            rows = slice(b, b + n - i)
            chi = numpy.stack([numpy.logspace(numpy.log10(float(r[2])), numpy.log10(float(r[3])),
                                              npts) for r in ranges[rows]])
            sigma = numpy.asarray(cosmo.sigma_r(chi.ravel(), 0.0),
                                  dtype=numpy.float64).reshape(chi.shape)
            ln_chi[rows] = numpy.log(chi)
            sigma2[rows] = sigma * sigma
            b += n - i
        return ln_chi, sigma2

    def get_covariance_batched(self, with_status=False, trispectrum=False, tabulated=False):
        """get_covariance() with every block in one device call: the same `wcovar`, and the same
        `covar` in every ``covariance_list[i][j - i]`` (the Poisson diagonal of the matching
        blocks included), bit for bit what the loop over fresh correlations returns.

        Blocks built with ssc_cov=True (all of them; with more than one correlation that means
        cross_terms=True) get the super-sample term as well: the epochs also carry the knot tables
        of the response (FAM_SSC), ONE more read-back gives every block's chi range
        (Context.covariance_ssc_blocks_range), the host lays the sigma^2 knots of every block
        (_ssc_blocks_knots: one MultiEpoch.sigma_r call per row of blocks), and
        Context.covariance_ssc_blocks runs kernel_ssc and covariance_ssc of every block in seven
        launches; its values ([n_blocks, n_pairs], kept in `self.blocks_ssc`; None without the
        term) are added to the Gaussian ones before the blocks are filled.  The
        batch builds neither the blocks' own KernelCovariance state (z_bar_NG, _kernel_ssc_array,
        ...) nor their HaloSuperSampleCovariance copies: it is what the loop returns for copies
        made from halos that had built no tables yet (a copy otherwise keeps the tables its halo
        had at construction, stale ones included; that is not reproduced).

        trispectrum=True opts in to the one-halo trispectrum term (without the keyword blocks
        built with nongaussian_cov=True are refused, as they always were).  Blocks built with
        nongaussian_cov=True (all of them, sharing one HaloTrispectrumOneHalo) then get
        covariance_NG as well: the trispectrum object's I_0^4 table is built if need be, on that
        object's own context, and ONE Context.covariance_ng_blocks call runs kernel_NG and
        covariance_NG of every block in eight launches, with no read-back and no sigma_r call.
        Its values ([n_blocks, n_pairs], kept in `self.blocks_ng`; None without the term) are
        added in the loop's order: Gaussian, then trispectrum, then super-sample.  An exhausted
        divmax of block (i, j) shows as ST_COV_NG_DIVMAX in correlation i's status word.  As with
        the super-sample term the batch does not build the blocks' own KernelCovariance NG state
        (_kernel_array, ...).

        tabulated=True opts in to kernels with tabulated redshift distributions (dNdzInterpolation,
        dNdChiGaussian: the photometric bins of a survey; without the keyword they are refused, as
        they always were).  The block kernels read the projection sets' tables only, so nothing
        but the set-up of the sets knows of it: a bin shared by several kernels is sent to the
        device once.

        The work: the correlations' kernels as projection sets on one kept grid.HaloGrid's context
        (Kernel._setup_pairs_on), ONE read-back of every kernel's z_bar -- the only
        synchronisation besides the result and the status words --, one HaloGrid epoch per
        correlation at its z_bar with its halo's cosmology and HOD, and Context.covariance_blocks:
        block (i, j) reads set i, set j, epoch i and epoch j where they lie.  The grid is kept,
        keyed as Correlation.correlation_kernels keys its own (rows, halo dictionary, mass
        function, the defaults a context snapshots).  The correlations, their kernels and their
        halos are not touched: unlike the loop (covariance.py:465-466) the batch does not move the
        halos to their z_bar, and it does not fill the blocks' own tables (_halo_a_array, ...).

        The status word of every correlation's epoch is read with the result, raised as a warning
        naming "correlation i", kept in `self.blocks_status` (uint32) beside `self.blocks_z_bar`
        and returned as the second element with with_status=True.

        ChompScopeError ("get_covariance_batched: <why>; use get_covariance", before any launch):
        nongaussian_cov without trispectrum=True, or poisson_noise_only; blocks that differ in
        ssc_cov or nongaussian_cov or do not share one halo_tri object and, with either term, in
        the k theta range or J0 limit of their KernelCovariance, or whose four windows have no
        redshift in common (the block is named); blocks whose power_spec, bins or areas differ; a
        kernel that is not exactly kernel.Kernel, has an assigned z_bar, a tabulated redshift
        distribution without tabulated=True, a w0-wa cosmology or another k theta range; a halo
        Correlation.correlation_hods would refuse, an HOD of another class, halos with different
        halo dictionaries or mass functions, two correlations sharing one Halo object; anything
        Covariance refuses for a cross block.  And, once z_bar is known: correlation 0's halo away
        from its z_bar (keep_halo_z_bar), which the loop's first block would be evaluated at."""
        import warnings
        from . import grid
        corrs, power_spec = self._batched_scope(trispectrum=trispectrum, tabulated=tabulated)
        n = len(corrs)
        halos = [c.halo for c in corrs]
        h0 = halos[0]
        kind = "tinker" if getattr(h0.mass, "_kind", 0) else "st"
        # (a context snapshots defaults.default_limits / default_precision when it is created)
        key = (n, tuple(sorted(h0.mass.halo_dict.items())), kind,
               tuple(sorted(defaults.default_limits.items())),
               tuple(sorted(defaults.default_precision.items())))
        kept = getattr(self, "_blocks_grid", (None, None))
        hg = kept[1] if kept[0] == key else None
        cosmos = [dict(h.cosmo.cosmo_dict) for h in halos]
        hods = [h.local_hod for h in halos]
        if hg is None:
            hg = grid.HaloGrid(numpy.zeros(n), cosmo_dict=cosmos, halo_dict=dict(h0.mass.halo_dict),
                               hod_dict=hods, mass_function=kind)
            self._blocks_grid = (key, hg)
        kernel_mod.Kernel._setup_pairs_on(hg.ctx, [c.kernel for c in corrs])
        z_bar = hg.ctx.kernel_info_sets()["z_bar"]       # (synchronises: z_bar per correlation)
        self.blocks_z_bar = z_bar
        if float(h0.get_redshift()) != float(z_bar[0]):
            raise _lib.ChompScopeError(
                "get_covariance_batched: the halo of correlation 0 is at z = %r, not at its "
                "kernel's z_bar = %r (keep_halo_z_bar): the loop evaluates the first block there; "
                "use get_covariance" % (float(h0.get_redshift()), float(z_bar[0])))
        blocks = [cov for row in self.covariance_list for cov in row]
        first = blocks[0]
        ssc = bool(first.ssc_cov)
        hg.set_parameters(cosmo=cosmos, z=z_bar, hod=hods)
        if ssc:      # (the response's knot tables h_m, pp_mm, I_1^2 beside the spectrum's own)
            hg.setup(power_spec, families=_lib.FAM_SSC)
        else:
            hg.setup(power_spec)
        nb = len(first.annular_bins)
        iu = numpy.triu_indices(nb)
        centers = numpy.array([b.center for b in first.annular_bins])
        code = h0._power_code(_POWER[power_spec][0])
        vals = hg.ctx.covariance_blocks(
            code, numpy.arange(n), first._j0_limit, first.area,
            [[cov.proj_power_poisson(p) for p in range(4)] for cov in blocks],
            centers[iu[0]], centers[iu[1]])
        self.blocks_ng = None
        if first.nongaussian_cov and nb:
            tri = first.halo_tri
            if not tri._initialized_i_0_4:
                tri._initialize_i_0_4()                      # (on the trispectrum object's own context)
            k0 = first.kernel
            self.blocks_ng = hg.ctx.covariance_ng_blocks(
                numpy.arange(n), k0.ln_ktheta_min, k0.ln_ktheta_max, k0._j0_limit, first.area,
                tri._i_0_4_array, tri._k_min, tri._k_max, centers[iu[0]], centers[iu[1]])
            vals = vals + self.blocks_ng                     # (the loop's order, get_covariance)
        self.blocks_ssc = None
        if ssc and nb:
            ranges = hg.ctx.covariance_ssc_blocks_range(n)   # (synchronises: chi range per block)
            ln_chi, sigma2 = self._ssc_blocks_knots([c.kernel.cosmo for c in corrs], ranges)
            k0 = first.kernel
            self.blocks_ssc = hg.ctx.covariance_ssc_blocks(
                numpy.arange(n), k0.ln_ktheta_min, k0.ln_ktheta_max, k0._j0_ssc_limit, ln_chi,
                sigma2, first.area, centers[iu[0]], centers[iu[1]])
            vals = vals + self.blocks_ssc                    # (the loop's order, get_covariance)
        words = hg.status()                              # (synchronises: the words of this result)
        self.blocks_status = words
        for cov, v in zip(blocks, vals):
            cov._fill_covar(v if nb else None)
        for i, w in enumerate(words):
            w = int(w)
            if w:
                category = (_lib.ChompParityWarning
                            if w & (_lib.ST_SATURATED | _lib.ST_MASS_SEARCH_EXHAUSTED)
                            else _lib.ChompAccuracyWarning)
                warnings.warn("correlation %d: %s" % (i, "; ".join(_lib.describe_status(w))),
                              category, stacklevel=2)
        self._assemble()
        return (self.wcovar, words) if with_status else self.wcovar


class CovarianceFourier(object):
    """covariance.py:874-1083: the Gaussian covariance of C_l.  Four Limber spectra over ln l,
    one per window pair X = a1a2, b1b2, a1b2, b1a2, each P_mm at that pair's z_bar:
    ``covariance_G(l) = (pl_a1a2 pl_b1b2 + pl_a1b2 pl_b1a2) / (2 l + 1)``.

    Reproduced as shipped, quirks included: z_bar is the first argmax of w1 w2 / chi^2 D^2 on
    linspace(min z_min_X, max z_max_X, kernel_npoints) (:1067-1075; windows that reach down to
    window_precision put it at the first grid point); the norms take the windows a1 and a2
    whatever the pair, l = chi (k = 1) and halo_a1a2's spectrum for a1b2 (:987-1006); the tables
    are integral / D(z_bar)^2 with the norm still in (:1048-1063), so _pl_X is C_l / D(z_bar)^2;
    ``covariance(l_a, l_b)`` is empty and returns None; ``input_halo`` itself is halo_a1a2 and is
    moved to z_bar_a1a2.  The two print statements are dropped.

    One deviation: the reference's other three halos are ``copy(input_halo)``, shallow copies that
    share one MassFunction which every set_redshift moves (halo.py:159), so with four different
    z_bar each halo integrates its tables with the mass function of the last redshift set.  Here
    the four are independent epochs (deep-copy semantics); where the z_bar coincide the two agree.

    Only the four windows and the MultiEpoch of the KernelCovariance are read: neither kernel_ssc
    nor kernel_NG is built, whatever its ``four_windows``.  Outside the scope (ChompScopeError,
    before anything is launched): no KernelCovariance, an ``input_halo`` that is not exactly a
    halo.Halo with an NFW profile, a pair of windows with no redshift in common."""

    _PAIRS = ("a1a2", "b1b2", "a1b2", "b1a2")

    def __init__(self, l_min, l_max, input_kernel_covariance=None, input_halo=None,
                 input_halo_trispectrum=None, **kws):
        if input_kernel_covariance is None:
            raise _lib.ChompScopeError(
                "CovarianceFourier needs a KernelCovariance (input_kernel_covariance): the "
                "reference's default, None, fails at its first attribute (covariance.py:887)")
        if type(input_halo) is not halo_mod.Halo or input_halo._general_profile:
            raise _lib.ChompScopeError(
                "CovarianceFourier is accelerated for an input_halo that is exactly a chomp_amd "
                "halo.Halo with an NFW profile, not %s: its four spectra are four epochs of one "
                "halo model" % ("a general_profile Halo" if type(input_halo) is halo_mod.Halo
                                else type(input_halo).__name__))
        self._ln_l_min = numpy.log(l_min)
        self._ln_l_max = numpy.log(l_max)
        self._ln_l_array = numpy.linspace(self._ln_l_min, self._ln_l_max,
                                          defaults.default_precision["corr_npoints"])
        self.kernel = input_kernel_covariance
        self._refresh_ranges()
        self.window_a1 = self.kernel.window_function_a1.window_function
        self.window_a2 = self.kernel.window_function_a2.window_function
        self.window_b1 = self.kernel.window_function_b1.window_function
        self.window_b2 = self.kernel.window_function_b2.window_function
        self.halo_a1a2 = input_halo
        self.halo_tri = input_halo_trispectrum
        self._initialized_pl = False
        self._table_key = None
        self._side_kernels = None

    def _windows(self):
        k = self.kernel
        return (k.window_function_a1, k.window_function_a2, k.window_function_b1,
                k.window_function_b2)

    def _refresh_ranges(self):
        """covariance.py:887-910 (the reference sets these once, at construction; here they follow
        the windows, so that the tables after a change are those of a new object)."""
        a1, a2, b1, b2 = self._windows()
        for name, (w1, w2) in zip(self._PAIRS, ((a1, a2), (b1, b2), (a1, b2), (b1, a2))):
            z_min, z_max = numpy.max([w1.z_min, w2.z_min]), numpy.min([w1.z_max, w2.z_max])
            if not z_min < z_max:
                raise _lib.ChompScopeError(
                    "CovarianceFourier: the windows of pair %s have no redshift in common (z_min "
                    "= %g >= z_max = %g)" % (name, z_min, z_max))
            setattr(self, "_z_min_" + name, z_min)
            setattr(self, "_z_max_" + name, z_max)
        self._z_array = numpy.linspace(
            numpy.min([getattr(self, "_z_min_" + p) for p in self._PAIRS]),
            numpy.max([getattr(self, "_z_max_" + p) for p in self._PAIRS]),
            defaults.default_precision["kernel_npoints"])

    def _kernels(self):
        """Two Kernels of this object's own whose set-ups the two cross slots are staged from,
        windows only: (a1, a2) with the MultiEpoch, and (b1, b2)."""
        k = self.kernel
        if self._side_kernels is None or self._side_kernels[2] != self._windows() + (k.cosmo,):
            kt = (numpy.exp(k.ln_ktheta_min), numpy.exp(k.ln_ktheta_max))
            a1, a2, b1, b2 = self._windows()
            self._side_kernels = (kernel_mod.Kernel(kt[0], kt[1], a1, a2, k.cosmo),
                                  kernel_mod.Kernel(kt[0], kt[1], b1, b2, k.cosmo),
                                  self._windows() + (k.cosmo,))
        return self._side_kernels[:2]

    @staticmethod
    def _halo_key(h):
        """What P_mm of a halo is built from apart from its redshift, readable without the
        device (the HOD does not enter)."""
        return (id(h), tuple(sorted(h.cosmo.cosmo_dict.items())),
                bool(getattr(h.cosmo, "_with_bao", False)), tuple(sorted(h.mass.halo_dict.items())),
                h.mass._kind, repr(sorted(h._profile_dict.items())), h.get_extrapolation())

    def _tables(self):
        """The device state in input_halo's context -- z_bar, the four epochs, the knot tables
        and their splines -- rebuilt when anything it was built from has changed."""
        h = self.halo_a1a2
        if type(h) is not halo_mod.Halo or h._general_profile:
            raise _lib.ChompScopeError("CovarianceFourier: halo_a1a2 must be a halo.Halo (NFW)")
        ctx = h._context()
        ka, kb = self._kernels()
        cfg = ctx.config
        key = (id(ctx), ka._signature(), kb._signature(), self._halo_key(h), self._ln_l_min,
               self._ln_l_max, cfg.corr_npoints, cfg.kernel_npoints)
        if (key == self._table_key and self._initialized_pl and
                getattr(ctx, "_cov_fourier_owner", None) is self):
            return ctx
        self._initialized_pl = False
        self._refresh_ranges()
        bao = bool(getattr(h.cosmo, "_with_bao", False))
        for c in (ctx, ka._dev(), kb._dev()):
            c.set_transfer(bao)
        # (whoever owned the slots stages again when it next needs them)
        ctx._cov_cross_owner = self
        ctx.covariance_cross_stage(0, ka._dev(), _lib.CROSS_WINDOWS)
        ctx.covariance_cross_stage(1, kb._dev(), _lib.CROSS_WINDOWS)
        info = ctx.covariance_fourier_zbar(self._z_array)
        z_bar = [float(v) for v in info[:, 2]]
        for p, z in zip(self._PAIRS, z_bar):
            setattr(self, "_z_bar_G_" + p, z)
        self._pl_scalars = info
        # covariance.py:968-971, with four independent halos: one epoch per distinct z_bar,
        # input_halo's own first
        h.set_redshift(z_bar[0])
        distinct = sorted(set(z_bar), key=z_bar.index)
        if len(distinct) == 1:
            h._sync(_lib.FAM_MM)
        else:
            h._sync_epochs(distinct, _lib.FAM_MM)
        epochs = [distinct.index(z) for z in z_bar]
        norms, tab, lev = ctx.covariance_fourier_table(h._power_code(_lib.P_MM), epochs,
                                                       self._ln_l_array)
        for i, p in enumerate(self._PAIRS):
            if not (numpy.isfinite(norms[i]) and norms[i] > 0.0):
                raise ValueError(
                    "CovarianceFourier._initialize_pl: the norm integrand of pair %s -- a1 a2 "
                    "D^2 / chi^2 P_mm(k = 1) at chi(z_bar = %g) (covariance.py:987-1006) -- is "
                    "not positive and finite (norm = %r): the windows a1 and a2 do not both "
                    "cover that redshift; the reference's table would be inf / NaN"
                    % (p, z_bar[i], float(norms[i])))
        for i, p in enumerate(self._PAIRS):
            setattr(self, "_norm_G_" + p, float(norms[i]))
            self.__dict__["_pl_%s_array" % p] = tab[i]
            self.__dict__["_pl_%s_levels" % p] = lev[i]
        self._table_key = key
        self._initialized_pl = True
        ctx._cov_fourier_owner = self
        return ctx

    def _initialize_pl(self):
        self._initialized_pl = False
        self._tables()

    def _calculate_zbar(self, window1, window2):
        """covariance.py:1067-1075 for two of this object's windows (the bound window_function
        methods the reference passes, or the window objects)."""
        ws = self._windows()
        owners = [getattr(w, "__self__", w) for w in (window1, window2)]
        for i, p in enumerate(((0, 1), (2, 3), (0, 3), (2, 1))):
            if owners[0] is ws[p[0]] and owners[1] is ws[p[1]]:
                self._tables()
                return getattr(self, "_z_bar_G_" + self._PAIRS[i])
        raise _lib.ChompScopeError(
            "_calculate_zbar is served for the four pairs of this object's windows: (a1, a2), "
            "(b1, b2), (a1, b2), (b1, a2)")

    def _evaluate(self, l):
        """[5, n] of a flat multipole array: the four _pl_X and covariance_G.  The logarithm and
        so the range rule are numpy's, on the host (covariance.py:935-938)."""
        ctx = self._tables()
        if _lib._is_torch(l):
            import torch
            lh = l.detach().cpu().numpy().astype(numpy.float64).ravel()
            with numpy.errstate(all="ignore"):
                x = numpy.concatenate([numpy.log(lh), lh])
            return ctx.covariance_fourier_gaussian(torch.as_tensor(x, device=l.device))
        lh = numpy.ascontiguousarray(l, dtype=numpy.float64).ravel()
        with numpy.errstate(all="ignore"):
            x = numpy.concatenate([numpy.log(lh), lh])
        if lh.size == 0:
            return numpy.empty((5, 0))
        return ctx.covariance_fourier_gaussian(x)

    def _row(self, row, l):
        if _lib._is_torch(l):
            return self._evaluate(l)[row].reshape(l.shape)
        la = numpy.asarray(l, dtype=numpy.float64)
        out = self._evaluate(la)[row]
        return float(out[0]) if la.ndim == 0 else out.reshape(la.shape)

    def _pl_a1a2(self, l):
        return self._row(0, l)

    def _pl_b1b2(self, l):
        return self._row(1, l)

    def _pl_a1b2(self, l):
        return self._row(2, l)

    def _pl_b1a2(self, l):
        return self._row(3, l)

    def covariance_G(self, l):
        """covariance.py:928-932.  A scalar gives a float, an array an array of its shape; a
        float64 torch cuda tensor gives a tensor on its device."""
        return self._row(4, l)

    def covariance(self, l_a, l_b):
        """covariance.py:925-926: empty in the reference."""
        return None


class FiniteAreaEffect(object):
    """Fitting formula for the finite-survey-area correction of Sato et al. 2011, App. A
    (covariance.py:1106-1139): two power laws in the source redshift; host arithmetic."""

    def __init__(self):
        self.alpha1 = 3.2952
        self.alpha2 = -0.316369
        self.beta1 = 0.170708
        self.beta2 = -0.349913

    def alpha(self, zs):
        return self.alpha1 * zs ** self.alpha2

    def beta(self, zs):
        return self.beta1 * zs ** self.beta2

    def area_scaling(self, area, zs):
        return self.alpha(zs) / area ** self.beta(zs)
