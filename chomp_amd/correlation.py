"""correlation.Correlation / CorrelationFourier / Correlation3d with the reference's
constructors and methods (correlation.py:33-289, 297-405, 408-510): one Romberg integral
per theta or r (over ln k) or per multipole (Limber, over chi), each on its own group of
wavefronts.
"""
import numpy

from . import _lib
from . import halo as halo_mod

speed_of_light = 3 * 10 ** 5
deg_to_rad = numpy.pi / 180.0
rad_to_deg = 180.0 / numpy.pi

_POWER = {"linear_power": (_lib.P_LIN, 0), "power_mm": (_lib.P_MM, _lib.FAM_MM),
          "power_gm": (_lib.P_GM, _lib.FAM_GM), "power_mg": (_lib.P_GM, _lib.FAM_GM),
          "power_gg": (_lib.P_GG, _lib.FAM_GG)}


class Correlation(object):
    """w(theta) (correlation.py:33-289)."""

    def __init__(self, theta_min_deg, theta_max_deg, input_kernel,
                 bins_per_decade=5.0, input_halo=None, power_spec=None,
                 k_min=None, k_max=None, keep_halo_z_bar=False, **kws):
        self.log_theta_min = numpy.log10(theta_min_deg * deg_to_rad)
        self.log_theta_max = numpy.log10(theta_max_deg * deg_to_rad)
        theta_array = []
        unit_double = numpy.floor(self.log_theta_min) * bins_per_decade
        theta = numpy.power(10.0, unit_double / (1.0 * bins_per_decade))
        while theta < numpy.power(10.0, self.log_theta_max):
            if (theta >= numpy.power(10.0, self.log_theta_min) and
                    theta < numpy.power(10.0, self.log_theta_max)):
                theta_array.append(10 ** (0.5 * (
                    numpy.log10(theta) + (unit_double + 1.0) / (1.0 * bins_per_decade))))
            unit_double += 1.0
            theta = numpy.power(10.0, unit_double / (1.0 * bins_per_decade))
        self.theta_array = numpy.array(theta_array)
        if theta_min_deg == theta_max_deg:
            self.theta_array = numpy.array([theta_min_deg * deg_to_rad])
        self.wtheta_array = numpy.zeros(self.theta_array.size)
        self.kernel = input_kernel
        if input_halo is None:
            input_halo = halo_mod.Halo(self.kernel.z_bar)
        self.halo = input_halo
        self.D_z = self._growth_at_z_bar()
        if not keep_halo_z_bar:
            self.halo.set_redshift(self.kernel.z_bar)
        if ((k_min is not None and k_min < self.halo._k_min) or
                (k_max is not None and k_max > self.halo._k_max)):
            self.halo.set_extrapolation(True)
        if k_min is None:
            k_min = self.halo._k_min
        self._ln_k_min = numpy.log(k_min)
        if k_max is None:
            k_max = self.halo._k_max
        self._ln_k_max = numpy.log(k_max)
        self._k_lim = (float(k_min), float(k_max))
        self.set_power_spectrum(power_spec)

    def _growth_at_z_bar(self):
        if self.kernel._z_bar_override is None:
            return self.kernel._get("D_zbar")
        return float(self.kernel.cosmo.growth_factor(self.kernel.z_bar))

    def get_redshift(self):
        return self.kernel.z_bar

    def set_redshift(self, redshift):
        self.kernel.z_bar = redshift
        self.D_z = self._growth_at_z_bar()
        self.halo.set_redshift(self.kernel.z_bar)

    def get_cosmology(self):
        return self.kernel.get_cosmology()

    def set_cosmology(self, cosmo_dict):
        self.kernel.set_cosmology(cosmo_dict)
        self.D_z = self._growth_at_z_bar()
        self.halo.set_cosmology(cosmo_dict, self.kernel.z_bar)

    def get_power_spectrum(self):
        return self._power_name

    def set_power_spectrum(self, powSpec):
        if powSpec is None:
            powSpec = 'linear_power'
        if powSpec not in _POWER or not hasattr(self.halo, powSpec):
            print("WARNING: Invalid input for power spectra variable,")
            print("\t setting to linear_power")
            powSpec = 'linear_power'
        self._power_name = powSpec
        self.power_spec = getattr(self.halo, powSpec)

    def get_halo(self):
        return self.halo.get_halo()

    def set_halo(self, halo_dict):
        self.halo.set_halo(halo_dict)

    def get_hod(self, return_object=False):
        return self.halo.get_hod(return_object)

    def set_hod(self, hod_dict):
        self.halo.set_hod(hod_dict)

    def set_hod_object(self, input_hod):
        self.halo.set_hod_object(input_hod)

    def _prepare(self, power_name=None, defer_status=False):
        """Halo tables and projection tables in ONE device context.  defer_status: see
        Halo._sync (the device-resident evaluation path synchronises nowhere)."""
        code, need = _POWER[self._power_name if power_name is None else power_name]
        # The projection tables first: their set-up runs on the context's side stream, beside
        # the halo set-up queued next (neither needs anything of the other).
        self.kernel._setup_on(self.halo._context())
        if isinstance(self.halo, halo_mod.HaloFit) and code != _lib.P_LIN:
            code |= _lib.P_HALOFIT
            if (code & 15) == _lib.P_MM:
                need = 0
            ctx = self.halo._ensure_halofit(need, defer_status=defer_status)
        else:
            ctx = self.halo._sync(need, defer_status=defer_status)
        return ctx, self.halo._power_code(code)

    def compute_correlation(self):
        self.wtheta_array = numpy.asarray(self.correlation(self.theta_array))

    def correlation(self, theta_rad):
        th = numpy.asarray(theta_rad, dtype=numpy.float64)
        ctx, code = self._prepare(defer_status=True)
        out = ctx.wtheta(code, 0, self._k_lim[0], self._k_lim[1], self.D_z,
                         numpy.ascontiguousarray(th).ravel())
        self.halo._resolve_status()            # (the result is on the host: nothing to hide)
        return float(out[0]) if th.ndim == 0 else out.reshape(th.shape)

    # -- the batch over HODs ---------------------------------------------------
    _hods_export = "chomp_wtheta_epochs"      # (the C entry point behind correlation_hods)

    def _hods_scope(self, hods=None, who="correlation_hods",
                    loop="set_hod / set_hod_object + correlation"):
        """ChompScopeError unless correlation_hods serves this object (and `hods`); no device
        work.  Returns the HODs as objects.  who / loop: the batch that asks and the loop it
        names instead (correlation_cosmologies shares this scope)."""
        from . import hod as hod_mod
        h = self.halo

        def refuse(why):
            raise _lib.ChompScopeError("%s: %s; use the loop %s" % (who, why, loop))
        if type(h) is not halo_mod.Halo:
            refuse("the halo is a %s, the batch takes a plain halo.Halo" % type(h).__name__)
        if getattr(h, "_general_profile", False):
            refuse("a general_profile halo (HaloGrid batches NFW epochs)")
        if h.get_extrapolation():
            refuse("an extrapolated spectrum (%s takes none)" % self._hods_export)
        if getattr(h.cosmo, "_with_bao", False):
            refuse("a with_bao cosmology")
        # HaloGrid's epochs take ONE halo dictionary for the mass function and the profile; after
        # set_halo the two of a Halo differ (halo.py:220-235)
        prof, mass = h._profile(), h.mass.halo_dict
        if any(prof.get(key) != mass.get(key) for key in set(prof) | set(mass)):
            refuse("the halo's profile and mass-function dictionaries differ (after set_halo)")
        objs = []
        for i, one in enumerate(hods if hods is not None else ()):
            if isinstance(one, dict):
                one = hod_mod.HODZheng(one)
            if type(one) not in (hod_mod.HODZheng, hod_mod.HODMandelbaum):
                refuse("hods[%d] is a %s, not a dictionary, HODZheng or HODMandelbaum"
                       % (i, type(one).__name__))
            objs.append(one)
        return objs

    def correlation_hods(self, theta_rad, hods, with_status=False):
        """w(theta) for many HODs in one call (on a CorrelationFourier: C_l, theta_rad being l;
        the two classes differ in _hods_evaluate alone): the array [len(hods), theta.size] whose row i is
        what set_hod_object(<hods[i] as an object>) followed by correlation(theta_rad) returns on
        a fresh Halo -- the loop of the reference's example script (example_script.py:141-143)
        as one batch.  hods: HOD dictionaries (HODZheng's) or hod.HODZheng / hod.HODMandelbaum
        objects, mixed freely.  This object's own halo and HOD are not touched.

        Every HOD is one epoch of one grid.HaloGrid at the halo's redshift (the kernel's z_bar)
        with the halo's cosmology, mass function and halo dictionary; the Kernel is staged on the
        grid's context and Context.wtheta_epochs evaluates all rows.  The grid is kept, keyed by
        what it was built from (the number of HODs, redshift, cosmology, halo dictionary, mass
        function and the defaults.default_limits / default_precision its context snapshots): a
        later call with the same key only replaces the HODs.  The grid's context stays on the
        device and stream it was created on.  The Kernel is not left as it was: staging it on the
        grid's context makes that context the one its later read-backs (z_bar, chi_min, ...) are
        served from, and the kernel keeps the context alive; its numbers do not change.

        The set-up's status word of every point is read with the result, raised as a
        ChompAccuracyWarning / ChompParityWarning naming the point, kept in
        `self.hods_status` (uint32 [len(hods)]) and returned as the second element with
        with_status=True.  A torch cuda theta returns a tensor.

        ChompScopeError (before any launch): a halo that is not exactly halo.Halo, a
        general_profile halo, extrapolation, with_bao, a halo whose profile and mass-function
        dictionaries differ (after set_halo), an HOD of another class."""
        return self._hods_batch(theta_rad, self._hods_scope(hods), with_status)

    def _hods_batch(self, theta_rad, objs, with_status):
        """correlation_hods behind its scope check (objs: _hods_scope's HOD objects): the kept
        grid, the set-up, _hods_evaluate and the status words.  Correlation3d.raw_correlation_hods
        shares it (theta_rad then being r)."""
        import warnings
        from . import grid
        n_hod = len(objs)
        th = theta_rad if _lib._is_torch(theta_rad) else numpy.asarray(theta_rad, dtype=numpy.float64)
        flat = th.reshape(-1) if _lib._is_torch(th) else numpy.ascontiguousarray(th).ravel()
        if n_hod == 0:
            out = flat.new_empty((0, flat.numel())) if _lib._is_torch(flat) else numpy.empty((0, flat.size))
            self.hods_status = numpy.zeros(0, dtype=numpy.uint32)
            return (out, self.hods_status) if with_status else out
        h = self.halo
        code, _ = _POWER[self._power_name]
        kind = "tinker" if getattr(h.mass, "_kind", 0) else "st"
        from . import defaults
        # (a context snapshots defaults.default_limits / default_precision when it is created)
        key = (n_hod, float(h.get_redshift()), tuple(sorted(h.cosmo.cosmo_dict.items())),
               tuple(sorted(h.mass.halo_dict.items())), kind,
               tuple(sorted(defaults.default_limits.items())),
               tuple(sorted(defaults.default_precision.items())))
        hg = self._hods_grid[1] if getattr(self, "_hods_grid", (None,))[0] == key else None
        if hg is None:
            hg = grid.HaloGrid(numpy.full(n_hod, h.get_redshift()), cosmo_dict=dict(h.cosmo.cosmo_dict),
                               halo_dict=dict(h.mass.halo_dict), hod_dict=objs, mass_function=kind)
            self._hods_grid = (key, hg)
        else:
            hg.set_parameters(hod=objs)
        self._hods_stage(hg.ctx)
        hg.setup(self._power_name)
        out = self._hods_evaluate(hg.ctx, h._power_code(code), n_hod, flat)
        words = hg.status()                    # (synchronises: the words belong to this result)
        self.hods_status = words
        for i, w in enumerate(words):
            w = int(w)
            if w:
                category = (_lib.ChompParityWarning
                            if w & (_lib.ST_SATURATED | _lib.ST_MASS_SEARCH_EXHAUSTED)
                            else _lib.ChompAccuracyWarning)
                warnings.warn("HOD %d: %s" % (i, "; ".join(_lib.describe_status(w))), category,
                              stacklevel=3)
        return (out, words) if with_status else out

    def _hods_stage(self, ctx):
        """What the batch needs on the grid's context besides the halo epochs: the Kernel's
        projection tables (queued before the halo set-up, on the context's side stream)."""
        self.kernel._setup_on(ctx)

    def _hods_evaluate(self, ctx, code, n_hod, flat):
        """The one call of correlation_hods that knows the observable: [n_hod, flat.size] of the
        grid's epochs 0 .. n_hod - 1 on its context."""
        return ctx.wtheta_epochs(code, 0, n_hod, self._k_lim[0], self._k_lim[1], self.D_z, flat)

    # -- the batch over cosmologies --------------------------------------------
    def _cosmologies_scope(self, cosmo_dicts, hods=None, tabulated=False, dark_energy=False):
        """ChompScopeError unless correlation_cosmologies serves this object, these cosmologies
        and `hods`; no device work.  tabulated / dark_energy: the caller's opt-ins, which let
        tabulated redshift distributions / w0-wa cosmologies through.  Returns the HODs as
        objects (None without `hods`)."""
        from . import cosmology
        from . import kernel as kernel_mod
        who, loop = "correlation_cosmologies", "set_cosmology (+ set_hod_object) + correlation"
        objs = self._hods_scope(hods, who=who, loop=loop)

        def refuse(why):
            raise _lib.ChompScopeError("%s: %s; use the loop %s" % (who, why, loop))
        if self.kernel._z_bar_override is not None:
            refuse("the kernel has an assigned z_bar (Correlation.set_redshift); the batch finds "
                   "z_bar per cosmology, as set_cosmology does")
        for name in ("window_function_a", "window_function_b"):
            dist = getattr(getattr(self.kernel, name, None), "_redshift_dist", None)
            if not tabulated and isinstance(dist, kernel_mod.dNdzInterpolation):
                refuse("%s has a tabulated redshift distribution (%s)" % (name, type(dist).__name__))
        for i, c in enumerate(cosmo_dicts):
            if not dark_energy and cosmology.has_dark_energy(c):
                refuse("cosmology %d has w0-wa dark energy" % i)
        if hods is not None and len(objs) != len(cosmo_dicts):
            raise ValueError("correlation_cosmologies: %d hods for %d cosmologies"
                             % (len(objs), len(cosmo_dicts)))
        return objs if hods is not None else None

    def correlation_cosmologies(self, theta_rad, cosmo_dicts, hods=None, with_status=False,
                                tabulated=False, dark_energy=False):
        """w(theta) for many cosmologies in one call: the array [len(cosmo_dicts), theta.size]
        whose row i is what set_cosmology(cosmo_dicts[i]) followed by correlation(theta_rad)
        returns on a fresh Correlation of the same kernel, halo parameters and HOD -- the loop
        of a cosmology design (correlation.py:161-171 and kernel.py:657-676 per point of
        simulation_design.py:116-155) as one batch.  With `hods` (one per point: dictionaries,
        hod.HODZheng or hod.HODMandelbaum, as in correlation_hods) set_hod_object(hods[i]) is
        applied as well.  This object's own kernel, halo, cosmology and HOD are not touched.

        The work: one projection set-up per point on the kept grid's context
        (Kernel._setup_sets_on), ONE read-back of every point's z_bar and D(z_bar) -- the only
        synchronisation besides the result and the status words --, one grid.HaloGrid epoch per
        point at z = z_bar[i] with cosmo_dicts[i], and Context.wtheta_sets.  As in the loop
        (set_cosmology moves the halo to the new z_bar, whatever keep_halo_z_bar said at
        construction) the batch ALWAYS evaluates the halo at z_bar[i].  The grid is kept, keyed by
        the number of points, the halo dictionary, the mass function and the defaults a context
        snapshots: a later call replaces cosmologies, redshifts and HODs only.  More points than
        _lib.KERNEL_SETS_MAX are worked off in blocks of that size.

        The status word of every point is read with the result, raised as a warning naming
        "cosmology i", kept in `self.cosmologies_status` (uint32) beside
        `self.cosmologies_z_bar` / `self.cosmologies_D_z` (the redshifts found and D there) and returned as the second element with
        with_status=True.  A torch cuda theta returns a tensor.

        tabulated=True takes dNdzInterpolation / dNdChiGaussian windows (a dNdChiGaussian keeps
        the table it was built with in every row, as in the loop), dark_energy=True takes w0-wa
        cosmologies among the points (Lambda-CDM points beside them compute what they compute
        in a Lambda-CDM batch).  Both are opt-ins of this call alone.

        ChompScopeError (before any launch): everything correlation_hods refuses, a kernel with
        an assigned z_bar (after set_redshift), without tabulated=True a dNdzInterpolation /
        dNdChiGaussian window, without dark_energy=True a w0-wa cosmology among the points.
        C_l (CorrelationFourier) is not batched over cosmologies yet."""
        cosmo_dicts = [dict(c) for c in cosmo_dicts]
        objs = self._cosmologies_scope(cosmo_dicts, hods, tabulated=tabulated,
                                       dark_energy=dark_energy)
        return self._sets_batch(
            theta_rad, "cosmologies", "cosmology", len(cosmo_dicts), objs, with_status,
            lambda b0, n: cosmo_dicts[b0:b0 + n],
            lambda ctx, b0, n: self.kernel._setup_sets_on(ctx, cosmo_dicts[b0:b0 + n]))

    def _sets_batch(self, theta_rad, name, label, n_pt, objs, with_status, cosmos_of, stage):
        """correlation_cosmologies and correlation_kernels behind their scope checks: n_pt rows,
        each one projection set and one grid.HaloGrid epoch at the set's z_bar, in blocks of
        _lib.KERNEL_SETS_MAX.  cosmos_of(b0, n): the cosmologies of rows b0 .. b0 + n - 1;
        stage(ctx, b0, n): their projection sets on the grid's context; objs: one HOD object per
        row, or None for this halo's HOD in every row.  The grid is kept in `_<name>_grid`, keyed
        by the rows of a block, the halo dictionary, the mass function and the defaults a context
        snapshots; the status words are kept in `<name>_status` beside `<name>_z_bar` and
        `<name>_D_z` and raised as warnings naming "<label> i"."""
        import warnings
        from . import defaults
        from . import grid
        th = theta_rad if _lib._is_torch(theta_rad) else numpy.asarray(theta_rad, dtype=numpy.float64)
        flat = th.reshape(-1) if _lib._is_torch(th) else numpy.ascontiguousarray(th).ravel()
        n_th = flat.numel() if _lib._is_torch(flat) else flat.size
        words, z_all, D_all = numpy.zeros(n_pt, dtype=numpy.uint32), numpy.zeros(n_pt), numpy.zeros(n_pt)
        setattr(self, name + "_status", words)
        setattr(self, name + "_z_bar", z_all)
        setattr(self, name + "_D_z", D_all)
        if n_pt == 0 or n_th == 0:
            out = flat.new_empty((n_pt, n_th)) if _lib._is_torch(flat) else numpy.empty((n_pt, n_th))
            return (out, words) if with_status else out
        h = self.halo
        code, _ = _POWER[self._power_name]
        kind = "tinker" if getattr(h.mass, "_kind", 0) else "st"
        rows = []
        for b0 in range(0, n_pt, _lib.KERNEL_SETS_MAX):
            n = min(_lib.KERNEL_SETS_MAX, n_pt - b0)
            cosmos = cosmos_of(b0, n)
            block_hods = list(objs[b0:b0 + n]) if objs is not None else h.local_hod
            # (a context snapshots defaults.default_limits / default_precision when it is created)
            key = (n, tuple(sorted(h.mass.halo_dict.items())), kind,
                   tuple(sorted(defaults.default_limits.items())),
                   tuple(sorted(defaults.default_precision.items())))
            kept = getattr(self, "_%s_grid" % name, (None, None))
            hg = kept[1] if kept[0] == key else None
            if hg is None:
                hg = grid.HaloGrid(numpy.zeros(n), cosmo_dict=cosmos, halo_dict=dict(h.mass.halo_dict),
                                   hod_dict=block_hods, mass_function=kind)
                setattr(self, "_%s_grid" % name, (key, hg))
            stage(hg.ctx, b0, n)
            info = hg.ctx.kernel_info_sets()           # (synchronises: z_bar and D(z_bar) per row)
            z_bar, D_z = info["z_bar"], info["D_zbar"]
            hg.set_parameters(cosmo=cosmos, z=z_bar, hod=block_hods)
            hg.setup(self._power_name)
            rows.append(self._kernels_evaluate(hg.ctx, h._power_code(code), n, D_z, flat))
            words[b0:b0 + n] = hg.status()             # (synchronises: this block's words)
            z_all[b0:b0 + n] = z_bar
            D_all[b0:b0 + n] = D_z
        if len(rows) == 1:
            out = rows[0]
        elif _lib._is_torch(flat):
            import torch
            out = torch.cat(rows)
        else:
            out = numpy.concatenate(rows)
        for i, w in enumerate(words):
            w = int(w)
            if w:
                category = (_lib.ChompParityWarning
                            if w & (_lib.ST_SATURATED | _lib.ST_MASS_SEARCH_EXHAUSTED)
                            else _lib.ChompAccuracyWarning)
                warnings.warn("%s %d: %s" % (label, i, "; ".join(_lib.describe_status(w))), category,
                              stacklevel=3)
        return (out, words) if with_status else out

    # -- the batch over kernels -------------------------------------------------
    _KERNELS_LOOP = "fresh Correlation objects, one per kernel, + correlation"

    def _kernels_scope(self, kernels, hods=None, tabulated=False, dark_energy=False):
        """ChompScopeError unless correlation_kernels serves this object, these kernels and
        `hods`; no device work.  tabulated / dark_energy: the caller's opt-ins, which let
        tabulated redshift distributions / w0-wa cosmologies through.  Returns the HODs as
        objects (None without `hods`)."""
        from . import cosmology
        from . import kernel as kernel_mod
        who, loop = "correlation_kernels", self._KERNELS_LOOP
        objs = self._hods_scope(hods, who=who, loop=loop)

        def refuse(why):
            raise _lib.ChompScopeError("%s: %s; use the loop %s" % (who, why, loop))
        mine = type(self.kernel)
        if mine not in (kernel_mod.Kernel, kernel_mod.GalaxyGalaxyLensingKernel):
            refuse("this object's kernel is a %s, the batch takes Kernel or "
                   "GalaxyGalaxyLensingKernel" % mine.__name__)
        for i, k in enumerate(kernels):
            if type(k) is not mine:
                refuse("kernel %d is a %s, this object's kernel a %s (one Bessel order per call)"
                       % (i, type(k).__name__, mine.__name__))
            if tuple(k._ktheta) != tuple(self.kernel._ktheta):
                refuse("kernel %d has another k theta range than this object's kernel" % i)
            if k._z_bar_override is not None:
                refuse("kernel %d has an assigned z_bar (Correlation.set_redshift); the batch "
                       "finds z_bar per kernel" % i)
            for name in ("window_function_a", "window_function_b"):
                dist = getattr(getattr(k, name, None), "_redshift_dist", None)
                if not tabulated and isinstance(dist, kernel_mod.dNdzInterpolation):
                    refuse("kernel %d: %s has a tabulated redshift distribution (%s)"
                           % (i, name, type(dist).__name__))
            if not dark_energy and cosmology.has_dark_energy(k.cosmo.cosmo_dict):
                refuse("kernel %d has a w0-wa cosmology" % i)
        if hods is not None and len(objs) != len(kernels):
            raise ValueError("correlation_kernels: %d hods for %d kernels" % (len(objs), len(kernels)))
        return objs if hods is not None else None

    def correlation_kernels(self, theta_rad, kernels, hods=None, with_status=False,
                            tabulated=False, dark_energy=False):
        """w(theta) for many kernels in one call (on a CorrelationFourier: C_l, theta_rad being
        l; the two classes differ in _kernels_evaluate alone): the array [len(kernels),
        theta.size] whose row i is what a fresh object of this class, built on kernels[i] with a
        fresh halo.Halo of kernels[i]'s cosmology, this halo's halo dictionary and mass function,
        the HOD hods[i] (this halo's without `hods`), this object's power spectrum and (w(theta))
        k range, returns from correlation(theta_rad) -- the window pairs of a tomographic
        analysis (kernel.py:559-839, one Correlation each: correlation.py:33-289) as one batch.
        As the constructor does without keep_halo_z_bar, the halo of row i is evaluated at
        kernels[i].z_bar with D_z = D(z_bar).  This object's own kernel, halo, cosmology and HOD
        are not touched, nor are the kernels' own read-backs.

        The work: one projection set-up per kernel on the kept grid's context
        (Kernel._setup_pairs_on: windows, MultiEpoch range and cosmology are the kernel's own),
        ONE read-back of every row's z_bar and D(z_bar), one grid.HaloGrid epoch per row at
        z_bar[i] with kernels[i]'s cosmology, and _kernels_evaluate (Context.wtheta_sets).  The
        grid is kept, keyed as correlation_cosmologies' (rows, halo dictionary, mass function,
        the defaults a context snapshots).  More kernels than _lib.KERNEL_SETS_MAX are worked
        off in blocks of that size.

        The status word of every row is read with the result, raised as a warning naming
        "kernel i", kept in `self.kernels_status` (uint32) beside `self.kernels_z_bar` and
        `self.kernels_D_z`, and returned as the second element with with_status=True.  A torch
        cuda theta returns a tensor.

        tabulated=True takes kernels with dNdzInterpolation / dNdChiGaussian windows -- the
        photometric bins of a survey; a bin shared by several kernels is sent to the device once
        --, dark_energy=True kernels with a w0-wa cosmology.  Both are opt-ins of this call alone.

        ChompScopeError (before any launch): everything correlation_hods refuses, a kernel whose
        type is not exactly this object's kernel's (Kernel or GalaxyGalaxyLensingKernel), a
        kernel with another k theta range, a kernel with an assigned z_bar, without
        tabulated=True a dNdzInterpolation / dNdChiGaussian window, without dark_energy=True a
        w0-wa cosmology.  ValueError: `hods` of another length."""
        from . import kernel as kernel_mod
        kernels = list(kernels)
        objs = self._kernels_scope(kernels, hods, tabulated=tabulated, dark_energy=dark_energy)
        return self._sets_batch(
            theta_rad, "kernels", "kernel", len(kernels), objs, with_status,
            lambda b0, n: [dict(k.cosmo.cosmo_dict) for k in kernels[b0:b0 + n]],
            lambda ctx, b0, n: kernel_mod.Kernel._setup_pairs_on(ctx, kernels[b0:b0 + n]))

    def _kernels_evaluate(self, ctx, code, n, D_z, flat):
        """The one call of the batches over projection sets (correlation_kernels,
        correlation_cosmologies) that knows the observable: [n, flat.size], row e the grid's
        epoch e against the context's projection set e with growth D_z[e]."""
        return ctx.wtheta_sets(code, 0, n, self._k_lim[0], self._k_lim[1], D_z, flat)

    def write(self, output_file_name):
        with open(output_file_name, "w") as f:
            f.write("#ttype1 = theta [deg]\n#ttype2 = wtheta\n")
            for theta, wtheta in zip(self.theta_array, self.wtheta_array):
                f.write("%1.10g %1.10g\n" % (theta / deg_to_rad, wtheta))


class CorrelationProjectedComoving(Correlation):
    """Empty in the reference too (correlation.py:291-295)."""

    def __init__(self, r_min_Mpc, r_max_Mpc, input_kernel,
                 bins_per_decade=5.0, input_halo=None, power_spec=None, **kws):
        pass


class CorrelationFourier(Correlation):
    """Limber C_l (correlation.py:297-405)."""

    def __init__(self, l_min, l_max, input_kernel, input_halo=None, powSpec=None,
                 **kws):
        from . import defaults
        self.log_l_min = numpy.log10(l_min)
        self.log_l_max = numpy.log10(l_max)
        self.l_array = numpy.logspace(self.log_l_min, self.log_l_max,
                                      defaults.default_precision["corr_npoints"])
        if l_min == l_max:
            self.l_array = numpy.array([l_min])
        self.power_array = numpy.zeros(self.l_array.size, dtype='float64')
        self.kernel = input_kernel
        if input_halo is None:
            input_halo = halo_mod.Halo(self.kernel.z_bar)
        self.halo = input_halo
        self.D_z = self._growth_at_z_bar()
        self.halo.set_redshift(self.kernel.z_bar)
        self.set_power_spectrum(powSpec)

    def compute_correlation(self):
        self.power_array = numpy.asarray(self.correlation(self.l_array))

    def correlation(self, l):
        la = numpy.asarray(l, dtype=numpy.float64)
        ctx, code = self._prepare(defer_status=True)
        out = ctx.cell(code, 0, self.D_z, numpy.ascontiguousarray(la).ravel())
        self.halo._resolve_status()
        return float(out[0]) if la.ndim == 0 else out.reshape(la.shape)

    # -- the batch over HODs ---------------------------------------------------
    _hods_export = "chomp_cell_epochs"

    def _hods_evaluate(self, ctx, code, n_hod, flat):
        """correlation_hods(l, hods, with_status=False) is Correlation's, inherited whole -- the
        scope and its refusals, the kept HaloGrid and its key, the Kernel staged on the grid's
        context, the status words and `hods_status`, a tensor for a torch cuda l -- with this as
        its evaluating call: row i of the array [len(hods), l.size] is what
        set_hod_object(<hods[i] as an object>) followed by correlation(l) returns on a fresh Halo.
        Context.cell_epochs builds one chi-only node table per call and runs the epochs' spectrum
        tables and Romberg integrals with an epoch axis, each row bit for bit what Context.cell
        returns for that epoch."""
        return ctx.cell_epochs(code, 0, n_hod, self.D_z, flat)

    def _kernels_evaluate(self, ctx, code, n, D_z, flat):
        """correlation_kernels(l, kernels, hods=None, with_status=False, tabulated=False,
        dark_energy=False) is Correlation's,
        inherited whole, with this as its evaluating call: Context.cell_sets builds one chi-only
        node table per row (the set's windows, growth and chi range) and runs the rows' spectrum
        tables and Romberg integrals with a set axis, each row bit for bit what Context.cell
        returns after Context.kernel_setup of that kernel.  A kernel carries its cosmology, so
        this is also the batch of C_l over cosmologies."""
        return ctx.cell_sets(code, 0, n, D_z, flat)

    def correlation_cosmologies(self, l, cosmo_dicts, hods=None, with_status=False):
        """C_l is not batched over cosmologies yet: the chi-only node table of
        Context.cell_epochs belongs to one projection set-up, and a set axis on it is the
        follow-up to Correlation.correlation_cosmologies.  Raises ChompScopeError (it must never
        return w(theta))."""
        raise _lib.ChompScopeError(
            "CorrelationFourier.correlation_cosmologies: C_l over cosmologies is not batched yet "
            "(the follow-up: a set axis on chomp_cell_epochs' chi-only node table); use the loop "
            "set_cosmology + correlation")

    def write(self, output_file_name):
        with open(output_file_name, "w") as f:
            f.write("#ttype1 = l [deg]\n#ttype2 = power\n")
            for l, power in zip(self.l_array, self.power_array):
                f.write("%1.10f %1.10f\n" % (l, power))


class Correlation3d(Correlation):
    """xi(r) from a halo-model spectrum (correlation.py:408-510): corr_npoints
    log-spaced separations, one Romberg integral of k^2/(2 pi) P(k) J0(k r) each -- the
    cylindrical J0, as the reference has it -- and a cubic spline in r."""

    def __init__(self, r_min, r_max, redshift=0.0, input_halo=None, powSpec=None,
                 k_min=None, k_max=None):
        from . import defaults
        self.log_r_min = numpy.log10(r_min)
        self.log_r_max = numpy.log10(r_max)
        self.r_array = numpy.logspace(self.log_r_min, self.log_r_max,
                                      defaults.default_precision["corr_npoints"])
        if r_min == r_max:
            self.r_array = numpy.array([r_min])
        self.xi_array = numpy.zeros(self.r_array.size)
        if input_halo is None:
            input_halo = halo_mod.Halo(redshift)
        self.halo = input_halo
        self.halo.set_redshift(redshift)
        if ((k_min is not None or k_max is not None) and
                not self.halo.get_extrapolation() and
                (k_min < self.halo._k_min or k_max > self.halo._k_max)):
            self.halo.set_extrapolation(True)
        if k_min is None:
            k_min = self.halo._k_min
        self._ln_k_min = numpy.log(k_min)
        if k_max is None:
            k_max = self.halo._k_max
        self._ln_k_max = numpy.log(k_max)
        self._k_lim = (float(k_min), float(k_max))
        self.set_power_spectrum(powSpec)
        self.initialized_spline = False

    def _prepare(self):
        code, need = _POWER[self._power_name]
        if isinstance(self.halo, halo_mod.HaloFit) and code != _lib.P_LIN:
            self.halo._ensure_halofit()     # (xi(r) returns to the host: nothing to defer)
            code |= _lib.P_HALOFIT
            if (code & 15) == _lib.P_MM:
                need = 0
        return self.halo._sync(need), self.halo._power_code(code)

    def compute_correlation(self):
        self.xi_array = numpy.asarray(self.raw_correlation(self.r_array))
        self.initialized_spline = True

    def raw_correlation(self, r):
        ra = numpy.asarray(r, dtype=numpy.float64)
        ctx, code = self._prepare()
        out = ctx.xi3d(code, 0, self._k_lim[0], self._k_lim[1],
                       numpy.ascontiguousarray(ra).ravel())
        return float(out[0]) if ra.ndim == 0 else out.reshape(ra.shape)

    # -- the batches over HODs and cosmologies -----------------------------------
    # They are defined on raw_correlation: the reference never resets initialized_spline after
    # set_hod, so correlation(r) in a loop keeps returning the first point's spline.
    _hods_export = "chomp_xi3d_epochs"
    _HODS_LOOP = "set_hod / set_hod_object + raw_correlation"
    _COSMOLOGIES_LOOP = "fresh Correlation3d objects (+ set_hod_object) + raw_correlation"

    @staticmethod
    def _table_scope(who, loop):
        """Context.xi3d_epochs integrates from a node table of level 20 and has no route beyond."""
        from . import defaults
        if defaults.default_precision["divmax"] > 20:
            raise _lib.ChompScopeError(
                "%s: default_precision['divmax'] = %d exceeds the node table of %s (level 20); "
                "use the loop %s" % (who, defaults.default_precision["divmax"],
                                     Correlation3d._hods_export, loop))

    def _hods_stage(self, ctx):
        """xi(r) needs no projection set-up."""

    def _hods_evaluate(self, ctx, code, n_hod, flat):
        return ctx.xi3d_epochs(code, 0, n_hod, self._k_lim[0], self._k_lim[1], flat)

    def raw_correlation_hods(self, r, hods, with_status=False):
        """xi(r) for many HODs in one call: the array [len(hods), r.size] whose row i is what
        set_hod_object(<hods[i] as an object>) followed by raw_correlation(r) returns on a fresh
        Halo, bit for bit.  hods, the kept grid.HaloGrid (one epoch per HOD at the halo's
        redshift) and its key, the status words (`self.hods_status`, warnings naming "HOD i",
        with_status=True) and the ChompScopeErrors are those of Correlation.correlation_hods;
        the evaluating call is Context.xi3d_epochs: the r-independent factor of the integrand
        once per HOD on the Romberg nodes, then one launch over (r, HOD).  A
        default_precision['divmax'] above 20 is refused as well.  A torch cuda r returns a
        tensor.  This object's own halo and HOD are not touched."""
        who = "raw_correlation_hods"
        objs = self._hods_scope(hods, who=who, loop=self._HODS_LOOP)
        self._table_scope(who, self._HODS_LOOP)
        if not _lib._is_torch(r) and numpy.asarray(r).size == 0:
            self.hods_status = numpy.zeros(len(objs), dtype=numpy.uint32)
            out = numpy.empty((len(objs), 0))
            return (out, self.hods_status) if with_status else out
        return self._hods_batch(r, objs, with_status)

    def raw_correlation_cosmologies(self, r, cosmo_dicts, hods=None, with_status=False):
        """xi(r) for many cosmologies in one call: the array [len(cosmo_dicts), r.size] whose row
        i is what a fresh Correlation3d(..., redshift=z, input_halo=Halo(z, <hod>,
        SingleEpoch(z, cosmo_dicts[i])), powSpec=...) of this object's redshift, k range, halo
        parameters, mass function and HOD returns from raw_correlation(r), bit for bit.  With
        `hods` (one per point, as in raw_correlation_hods) point i has hods[i].  w0-wa
        cosmologies are in scope.

        One grid.HaloGrid epoch per point at the halo's redshift (xi(r) has no projection, hence
        no z_bar, no projection sets and no block limit) and one Context.xi3d_epochs call.  The
        grid is kept, keyed by the number of points, the halo dictionary, the mass function and
        the defaults a context snapshots.  The status word of every point is read with the
        result, raised as a warning naming "cosmology i", kept in `self.cosmologies_status`
        and returned as the second element with with_status=True.  A torch cuda r returns a
        tensor.  This object's own halo, cosmology and HOD are not touched.

        ChompScopeError (before any launch): everything raw_correlation_hods refuses.
        ValueError: `hods` of another length than cosmo_dicts."""
        import warnings
        from . import defaults
        from . import grid
        who = "raw_correlation_cosmologies"
        cosmo_dicts = [dict(c) for c in cosmo_dicts]
        objs = self._hods_scope(hods, who=who, loop=self._COSMOLOGIES_LOOP)
        self._table_scope(who, self._COSMOLOGIES_LOOP)
        if hods is not None and len(objs) != len(cosmo_dicts):
            raise ValueError("raw_correlation_cosmologies: %d hods for %d cosmologies"
                             % (len(objs), len(cosmo_dicts)))
        n_pt = len(cosmo_dicts)
        ra = r if _lib._is_torch(r) else numpy.asarray(r, dtype=numpy.float64)
        flat = ra.reshape(-1) if _lib._is_torch(ra) else numpy.ascontiguousarray(ra).ravel()
        n_r = flat.numel() if _lib._is_torch(flat) else flat.size
        self.cosmologies_status = numpy.zeros(n_pt, dtype=numpy.uint32)
        if n_pt == 0 or n_r == 0:
            out = flat.new_empty((n_pt, n_r)) if _lib._is_torch(flat) else numpy.empty((n_pt, n_r))
            return (out, self.cosmologies_status) if with_status else out
        h = self.halo
        code, _ = _POWER[self._power_name]
        kind = "tinker" if getattr(h.mass, "_kind", 0) else "st"
        point_hods = list(objs) if hods is not None else h.local_hod
        # (a context snapshots defaults.default_limits / default_precision when it is created)
        key = (n_pt, tuple(sorted(h.mass.halo_dict.items())), kind,
               tuple(sorted(defaults.default_limits.items())),
               tuple(sorted(defaults.default_precision.items())))
        kept = getattr(self, "_cosmologies_grid", (None, None))
        hg = kept[1] if kept[0] == key else None
        z = numpy.full(n_pt, float(h.get_redshift()))
        if hg is None:
            hg = grid.HaloGrid(z, cosmo_dict=cosmo_dicts, halo_dict=dict(h.mass.halo_dict),
                               hod_dict=point_hods, mass_function=kind)
            self._cosmologies_grid = (key, hg)
        else:
            hg.set_parameters(cosmo=cosmo_dicts, z=z, hod=point_hods)
        hg.setup(self._power_name)
        out = hg.ctx.xi3d_epochs(h._power_code(code), 0, n_pt, self._k_lim[0], self._k_lim[1], flat)
        words = hg.status()                    # (synchronises: the words belong to this result)
        self.cosmologies_status = words
        for i, w in enumerate(words):
            w = int(w)
            if w:
                category = (_lib.ChompParityWarning
                            if w & (_lib.ST_SATURATED | _lib.ST_MASS_SEARCH_EXHAUSTED)
                            else _lib.ChompAccuracyWarning)
                warnings.warn("cosmology %d: %s" % (i, "; ".join(_lib.describe_status(w))), category,
                              stacklevel=2)
        return (out, words) if with_status else out

    def correlation_hods(self, r, hods, with_status=False):
        """Correlation's batch of w(theta) does not apply to xi(r); ChompScopeError."""
        raise _lib.ChompScopeError(
            "Correlation3d.correlation_hods: xi(r) is batched on raw_correlation; use "
            "raw_correlation_hods (or raw_correlation_cosmologies for a batch over cosmologies)")

    def correlation_cosmologies(self, r, cosmo_dicts, hods=None, with_status=False):
        """Correlation's batch of w(theta) does not apply to xi(r); ChompScopeError."""
        raise _lib.ChompScopeError(
            "Correlation3d.correlation_cosmologies: xi(r) is batched on raw_correlation; use "
            "raw_correlation_cosmologies (or raw_correlation_hods for a batch over HODs)")

    def correlation_kernels(self, r, kernels, hods=None, with_status=False):
        """xi(r) has no projection, hence no kernels to batch over; ChompScopeError."""
        raise _lib.ChompScopeError(
            "Correlation3d.correlation_kernels: xi(r) has no projection kernel; use "
            "raw_correlation_hods or raw_correlation_cosmologies for the batches of xi(r)")

    def correlation(self, r):
        if not self.initialized_spline:
            self.compute_correlation()
        ra = numpy.asarray(r, dtype=numpy.float64)
        r_min, r_max = 10. ** self.log_r_min, 10. ** self.log_r_max
        inside = numpy.logical_and(ra <= r_max, ra > r_min)
        out = numpy.zeros(ra.shape)
        if numpy.any(inside):
            ctx, _ = self._prepare()
            out[inside] = ctx.spline_eval(self.r_array, self.xi_array, ra[inside])
        return out

    def write(self, output_file_name):
        with open(output_file_name, "w") as f:
            f.write("#ttype1 = r [Mpc/h]\n#ttype2 = xi\n")
            for r, xi in zip(self.r_array, self.xi_array):
                f.write("%1.10g %1.10g\n" % (r, xi))
