"""simulation_design.SimulationDesign with the reference's interface
(simulation_design.py:36-234): Latin-hypercube design points in parameter space, one model
evaluation per point, results in a pandas DataFrame.

The reference evaluates the points one after another through the object's
set_cosmology / set_halo / set_hod and the requested method.  That generic loop is kept
(it works with every chomp_amd object).  When the object is a Halo and the method one of
its spectra, the design is the native batch axis of the device library: every design
point becomes one epoch of a HaloGrid and all of them are built and evaluated by the same
kernel launches.  A design over HOD parameters of
Correlation.correlation or CorrelationFourier.correlation is batched the same way, through the
object's correlation_hods; a design over cosmology parameters of Correlation.correlation through
correlation_cosmologies, with run_design(batched="cosmology").  Designs over HOD or cosmology
parameters of Correlation3d.raw_correlation are batched on request (batched=True / "cosmology"),
through raw_correlation_hods / raw_correlation_cosmologies.
"""
import copy
import warnings

import numpy
import pandas

from . import _lib
from . import correlation as correlation_mod
from . import defaults
from . import grid
from . import halo as halo_mod
from . import hod as hod_mod

default_parameter_dict = {"cosmo_dict": defaults.default_cosmo_dict,
                          "halo_dict": defaults.default_halo_dict,
                          "hod_dict": defaults.default_hod_dict}

_BATCHED_METHODS = ("linear_power", "power_mm", "power_gm", "power_mg", "power_gg")


def _hod_dict_of(h):
    """The parameter dictionary of an HODZheng; one built without a dictionary keeps None
    (hod.py:157-165) and answers from its attributes."""
    d = h.get_hod()
    if d is None:
        d = {key: getattr(h, key) for key in ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")}
    return dict(d)


def _point_hod(local_hod, hod_dict):
    """The HOD of one design point for the batch, in the halo's own model: Halo.set_hod re-
    initialises the halo's HOD object from the point's dictionary (halo.py:181-192).  A Zheng HOD
    goes as its dictionary (HaloGrid reads that as HODZheng)."""
    if isinstance(local_hod, hod_mod.HODMandelbaum):
        return hod_mod.HODMandelbaum(hod_dict) if hod_dict is not None else local_hod
    return hod_dict if hod_dict is not None else _hod_dict_of(local_hod)


def random_lhs(n, k):
    """n points of a random Latin hypercube in k variables (what simulation_design.py:17-33 takes
    from the R package 'lhs'): every variable's range is cut into n strata, each stratum is used
    by exactly one point, and a point sits uniformly inside its stratum.  Draws from numpy's
    global generator in the reference's order (the k orderings first, then the positions), so a
    seeded design is the reference's design."""
    strata = numpy.empty((n, k), dtype=numpy.float64)
    for col in range(k):
        strata[:, col] = numpy.random.permutation(n)
    inside = numpy.random.uniform(size=(n, k))
    return (strata + inside) / float(n)


class _Recorder(object):
    """Stands in for the model object while the design's setters run: keeps the
    dictionaries they hand over instead of rebuilding a model per point."""

    def __init__(self):
        self.cosmo = self.halo = self.hod = None

    def set_cosmology(self, cosmo_dict, *args, **kws):
        self.cosmo = dict(cosmo_dict)

    def set_halo(self, halo_dict, *args, **kws):
        self.halo = dict(halo_dict)

    def set_hod(self, hod_dict, *args, **kws):
        self.hod = dict(hod_dict)


class SimulationDesign(object):
    """simulation_design.py:36-234.  params: {name: [center, min, max]} with names from
    the cosmology, halo or HOD dictionaries of defaults.py."""

    def __init__(self, input_chomp_object, method_name, params, n_design=100,
                 independent_var=None, default_param_dict=None):
        self._input_object = input_chomp_object
        self._method = method_name
        self.params = pandas.DataFrame(params, index=['center', 'min', 'max'])
        self.n_design = n_design
        self._ind_var = independent_var
        self._initialized_design = False
        if default_param_dict is None:
            default_param_dict = default_parameter_dict
        # (the reference mutates the caller's dictionaries point after point; a private
        # copy keeps the defaults of this process intact)
        self._default_param_dict = copy.deepcopy(default_param_dict)
        self._vary_cosmology = False
        self._vary_halo = False
        self._vary_hod = False
        self._param_types = []
        for key in self.params.keys():
            for kind, flag in (("cosmo_dict", "_vary_cosmology"), ("halo_dict", "_vary_halo"),
                               ("hod_dict", "_vary_hod")):
                if key in self._default_param_dict[kind]:
                    self._param_types.append(kind)
                    setattr(self, flag, True)
                    break

    def _init_design_points(self):
        """simulation_design.py:101-114."""
        diff = (self.params.xs('max') - self.params.xs('min')).rename('diff')
        self.params = pandas.concat([self.params, diff.to_frame().transpose()])
        points = pandas.DataFrame(random_lhs(self.n_design, self.params.shape[1]),
                                  columns=self.params.columns)
        self.lhs = points
        self.points = points * self.params.xs('diff') + self.params.xs('min')
        self._initialized_design = True

    def _apply_point(self, point):
        if self._vary_cosmology:
            self.set_cosmology(self._default_param_dict['cosmo_dict'], point)
        if self._vary_halo:
            self.set_halo(self._default_param_dict['halo_dict'], point)
        if self._vary_hod:
            self.set_hod(self._default_param_dict['hod_dict'], point)

    def _run_des_point(self, point):
        """simulation_design.py:116-138: one design point through the object's setters."""
        self._apply_point(point)
        if self._ind_var is None:
            values = getattr(self._input_object, self._method)()
        else:
            values = getattr(self._input_object, self._method)(self._ind_var)
        return pandas.Series(numpy.asarray(values).flatten())

    def _hods_design_scope(self):
        """ChompScopeError unless this design is one Correlation.correlation_hods serves: exactly a
        Correlation or a CorrelationFourier (any other subclass may evaluate something else under
        the same name), its `correlation` over an independent variable (theta; l of a
        CorrelationFourier), only HOD parameters varying
        (a cosmology point needs its own projection set-up, and a context holds one; halo
        parameters keep the loop as in the Halo route), and the object within correlation_hods'
        own scope.  No device work."""
        obj = self._input_object
        why = None
        if type(obj) not in (correlation_mod.Correlation, correlation_mod.CorrelationFourier):
            why = ("the object is a %s, not exactly a correlation.Correlation or "
                   "correlation.CorrelationFourier" % type(obj).__name__)
        elif self._method != "correlation":
            why = "the method is %r, not 'correlation'" % (self._method,)
        elif self._ind_var is None:
            why = "no independent_var (theta, or l of a CorrelationFourier) is given"
        elif not self._vary_hod:
            why = "no HOD parameter varies"
        elif self._vary_cosmology:
            why = "a cosmology parameter varies"
        elif self._vary_halo:
            why = "a halo parameter varies ('alpha' names the halo profile's slope first)"
        if why is not None:
            raise _lib.ChompScopeError("the batched design over Correlation.correlation_hods does "
                                       "not serve this design: %s; use batched=False" % why)
        obj._hods_scope()

    def _batched_route(self):
        """"halo" / "correlation": the batched route this design takes by itself; None: the loop."""
        if isinstance(self._input_object, correlation_mod.Correlation):
            try:
                self._hods_design_scope()
            except _lib.ChompScopeError:
                return None
            return "correlation"
        return "halo" if self._batched_halo() else None

    def _batched(self):
        return self._batched_route() is not None

    def _batched_halo(self):
        obj = self._input_object
        # Halo.set_halo only reaches the mass function and leaks into later points through
        # set_cosmology (halo.py:151-162, 220-235): designs over halo parameters keep the
        # point-by-point loop, which reproduces that.
        return (type(obj) is halo_mod.Halo and self._method in _BATCHED_METHODS and
                self._ind_var is not None and not self._vary_halo and
                not obj.get_extrapolation() and
                # (HaloGrid batches NFW epochs: a general-profile object keeps the loop)
                not getattr(obj, "_general_profile", False))

    def _run_batched(self):
        """Every design point = one epoch of one HaloGrid."""
        real, rec = self._input_object, _Recorder()
        obj = real
        cosmos, halos, hods = [], [], []
        self._input_object = rec
        try:
            for _, point in self.points.iterrows():
                rec.cosmo = rec.halo = rec.hod = None
                self._apply_point(point)
                cosmos.append(rec.cosmo if rec.cosmo is not None else dict(obj.cosmo.cosmo_dict))
                halos.append(dict(obj.mass.halo_dict))
                hods.append(_point_hod(obj.local_hod, rec.hod))
        finally:
            self._input_object = real
        kind = "tinker" if getattr(obj.mass, "_kind", 0) else "st"
        hg = grid.HaloGrid(numpy.full(len(cosmos), obj.get_redshift()), cosmo_dict=cosmos,
                           halo_dict=halos, hod_dict=hods, mass_function=kind)
        k = numpy.asarray(self._ind_var, dtype=numpy.float64)
        out = hg.power(self._method, k.ravel())
        # The result is on the host: read the status words now and say which design points they
        # concern.  What the point-by-point loop reports through Halo._sync (an exhausted divmax =
        # scipy's AccuracyWarning; a saturated mass-limit search, where the reference's own answer
        # is decided by rounding noise and may differ by percents) must not get lost in a batch.
        self._warn_design_status(hg.status(), stacklevel=4)
        return pandas.DataFrame(numpy.asarray(out).T, columns=self.points.index)

    def _warn_design_status(self, words, stacklevel):
        self.design_status = pandas.Series([int(w) for w in words], index=self.points.index,
                                           name="status", dtype="int64")
        for label, w in self.design_status.items():
            if w:
                category = (_lib.ChompParityWarning
                            if w & (_lib.ST_SATURATED | _lib.ST_MASS_SEARCH_EXHAUSTED)
                            else _lib.ChompAccuracyWarning)
                warnings.warn("design point %s: %s" % (label, "; ".join(_lib.describe_status(w))),
                              category, stacklevel=stacklevel)

    def _run_batched_hods(self):
        """Every design point = one HOD of one correlation_hods call (w(theta) of a Correlation,
        C_l of a CorrelationFourier: the independent variable is theta or l)."""
        real, rec = self._input_object, _Recorder()
        self._hods_design_scope()             # (ChompScopeError before anything is recorded)
        hods = []
        self._input_object = rec
        try:
            for _, point in self.points.iterrows():
                rec.cosmo = rec.halo = rec.hod = None
                self._apply_point(point)
                hods.append(_point_hod(real.halo.local_hod, rec.hod))
        finally:
            self._input_object = real
        theta = numpy.asarray(self._ind_var, dtype=numpy.float64)
        with warnings.catch_warnings():       # (raised below, naming the design point)
            warnings.simplefilter("ignore", _lib.ChompAccuracyWarning)
            warnings.simplefilter("ignore", _lib.ChompParityWarning)
            out, words = real.correlation_hods(theta.ravel(), hods, with_status=True)
        self._warn_design_status(words, stacklevel=4)
        return pandas.DataFrame(numpy.asarray(out).T, columns=self.points.index)

    def _cosmologies_design_scope(self):
        """ChompScopeError unless this design is one Correlation.correlation_cosmologies serves:
        exactly a Correlation, its `correlation` over an independent variable (theta), cosmology
        parameters varying (HOD parameters may vary with them), no halo parameter, and the object
        within correlation_cosmologies' own scope.  No device work."""
        obj = self._input_object
        why = None
        if type(obj) is not correlation_mod.Correlation:
            why = ("the object is a %s, not exactly a correlation.Correlation (C_l over cosmologies "
                   "is not batched yet)" % type(obj).__name__)
        elif self._method != "correlation":
            why = "the method is %r, not 'correlation'" % (self._method,)
        elif self._ind_var is None:
            why = "no independent_var (theta) is given"
        elif not self._vary_cosmology:
            why = "no cosmology parameter varies"
        elif self._vary_halo:
            why = "a halo parameter varies ('alpha' names the halo profile's slope first)"
        if why is not None:
            raise _lib.ChompScopeError("the batched design over Correlation.correlation_cosmologies "
                                       "does not serve this design: %s; use batched=False" % why)
        obj._cosmologies_scope([])

    def _run_batched_cosmologies(self):
        """Every design point = one cosmology (and, when HOD parameters vary, one HOD) of one
        correlation_cosmologies call: the loop of simulation_design.py:116-155 over
        Correlation.set_cosmology (correlation.py:161-171) as one batch."""
        real, rec = self._input_object, _Recorder()
        self._cosmologies_design_scope()      # (ChompScopeError before anything is recorded)
        cosmos, hods = [], []
        self._input_object = rec
        try:
            for _, point in self.points.iterrows():
                rec.cosmo = rec.halo = rec.hod = None
                self._apply_point(point)
                cosmos.append(rec.cosmo if rec.cosmo is not None
                              else dict(real.halo.cosmo.cosmo_dict))
                hods.append(_point_hod(real.halo.local_hod, rec.hod))
        finally:
            self._input_object = real
        theta = numpy.asarray(self._ind_var, dtype=numpy.float64)
        with warnings.catch_warnings():       # (raised below, naming the design point)
            warnings.simplefilter("ignore", _lib.ChompAccuracyWarning)
            warnings.simplefilter("ignore", _lib.ChompParityWarning)
            out, words = real.correlation_cosmologies(
                theta.ravel(), cosmos, hods=hods if self._vary_hod else None, with_status=True)
        self._warn_design_status(words, stacklevel=4)
        return pandas.DataFrame(numpy.asarray(out).T, columns=self.points.index)

    def _xi_design_scope(self, cosmology):
        """ChompScopeError unless this design is one Correlation3d.raw_correlation_hods
        (cosmology=False: only HOD parameters vary) or raw_correlation_cosmologies
        (cosmology=True: cosmology parameters vary, HOD parameters optionally with them) serves:
        the method 'raw_correlation' over an independent variable (r), no halo parameter, and the
        object within the batch's own scope.  No device work."""
        obj = self._input_object
        name = "raw_correlation_cosmologies" if cosmology else "raw_correlation_hods"
        why = None
        if self._method != "raw_correlation":
            why = ("the method is %r, not 'raw_correlation' (the reference's spline "
                   "correlation(r) keeps the first point's values in a loop)" % (self._method,))
        elif self._ind_var is None:
            why = "no independent_var (r) is given"
        elif cosmology and not self._vary_cosmology:
            why = "no cosmology parameter varies"
        elif not cosmology and not self._vary_hod:
            why = "no HOD parameter varies"
        elif not cosmology and self._vary_cosmology:
            why = "a cosmology parameter varies (batched='cosmology' serves that)"
        elif self._vary_halo:
            why = "a halo parameter varies ('alpha' names the halo profile's slope first)"
        if why is not None:
            raise _lib.ChompScopeError("the batched design over Correlation3d.%s does not serve "
                                       "this design: %s; use batched=False" % (name, why))
        obj._hods_scope(who=name, loop=obj._COSMOLOGIES_LOOP if cosmology else obj._HODS_LOOP)

    def _run_batched_xi(self, cosmology):
        """Every design point = one HOD of one Correlation3d.raw_correlation_hods call, or one
        cosmology (and, when HOD parameters vary, one HOD) of one raw_correlation_cosmologies
        call: the loop over the object's setters and raw_correlation(r) as one batch."""
        real, rec = self._input_object, _Recorder()
        self._xi_design_scope(cosmology)      # (ChompScopeError before anything is recorded)
        cosmos, hods = [], []
        self._input_object = rec
        try:
            for _, point in self.points.iterrows():
                rec.cosmo = rec.halo = rec.hod = None
                self._apply_point(point)
                cosmos.append(rec.cosmo if rec.cosmo is not None
                              else dict(real.halo.cosmo.cosmo_dict))
                hods.append(_point_hod(real.halo.local_hod, rec.hod))
        finally:
            self._input_object = real
        r = numpy.asarray(self._ind_var, dtype=numpy.float64)
        with warnings.catch_warnings():       # (raised below, naming the design point)
            warnings.simplefilter("ignore", _lib.ChompAccuracyWarning)
            warnings.simplefilter("ignore", _lib.ChompParityWarning)
            if cosmology:
                out, words = real.raw_correlation_cosmologies(
                    r.ravel(), cosmos, hods=hods if self._vary_hod else None, with_status=True)
            else:
                out, words = real.raw_correlation_hods(r.ravel(), hods, with_status=True)
        self._warn_design_status(words, stacklevel=4)
        return pandas.DataFrame(numpy.asarray(out).T, columns=self.points.index)

    def run_design(self, batched=None, with_status=False):
        """simulation_design.py:140-155.  Returns a DataFrame with one column per design
        point holding the flattened output of the method.  batched=None picks the
        one-launch path when the object / method allow it: a Halo and one of its spectra
        (cosmology and HOD may vary), or a Correlation or CorrelationFourier, its `correlation` and
        a design over HOD parameters only (the object's correlation_hods, with its scope).  A Correlation design
        that varies cosmology or halo parameters keeps the point-by-point loop: a cosmology
        point needs its own projection set-up, and a device context holds one.  batched=False
        forces the loop; batched=True on a Correlation raises ChompScopeError when the object
        or the design is outside that scope (nothing a point sets is ever dropped silently).

        The batched path keeps the status word of every design point (chomp_get_status bits) in
        `self.design_status` (an int64 Series indexed like the design points) and raises them as
        warnings naming the point; with_status=True returns the pair (frame, design_status) --
        the words are never mixed into the float frame, whose rows stay the method's output.

        batched="cosmology" (opt-in; None and True never pick it) evaluates a design over
        cosmology parameters -- HOD parameters optionally with them, no halo parameter -- of
        exactly a Correlation, its `correlation` and an independent variable by ONE
        Correlation.correlation_cosmologies call: one projection set-up and one halo epoch per
        point.  Outside that scope it raises ChompScopeError with the reason.

        An object that is exactly a Correlation3d is batched on request only (batched=None keeps
        its loop): with the method 'raw_correlation' and an independent variable (r),
        batched=True evaluates a design over HOD parameters by one raw_correlation_hods call and
        batched="cosmology" a design over cosmology (and HOD) parameters by one
        raw_correlation_cosmologies call; ChompScopeError outside that scope."""
        if not self._initialized_design:
            self._init_design_points()
        xi = type(self._input_object) is correlation_mod.Correlation3d
        if isinstance(batched, str):
            if batched != "cosmology":
                raise ValueError("run_design: batched=%r (None, True, False or 'cosmology')" % (batched,))
            self.design_status = None
            self.design_values = (self._run_batched_xi(True) if xi
                                  else self._run_batched_cosmologies())
            self.values_frame = self.design_values
            if with_status:
                return self.design_values, self.design_status
            return self.design_values
        if batched is None:
            batched = self._batched()
        self.design_status = None
        if batched and xi:
            self.design_values = self._run_batched_xi(False)
        elif batched:
            route = self._batched_route()
            if route is None:                  # (forced)
                route = ("correlation" if isinstance(self._input_object, correlation_mod.Correlation)
                         else "halo")
            self.design_values = (self._run_batched_hods() if route == "correlation"
                                  else self._run_batched())
        else:
            self.design_values = self.points.transpose().apply(self._run_des_point)
        self.values_frame = self.design_values
        if with_status:
            return self.design_values, self.design_status
        return self.design_values

    def set_cosmology(self, cosmo_dict=None, values=None):
        """simulation_design.py:157-175."""
        if cosmo_dict is None:
            cosmo_dict = self._default_param_dict['cosmo_dict']
        for key in self.params.keys():
            if key in cosmo_dict and key in values:
                cosmo_dict[key] = values[key]
        self._input_object.set_cosmology(cosmo_dict)

    def set_halo(self, halo_dict=None, values=None):
        """simulation_design.py:177-193."""
        if halo_dict is None:
            halo_dict = self._default_param_dict['halo_dict']
        for key in self.params.keys():
            if key in halo_dict and key in values:
                halo_dict[key] = values[key]
        self._input_object.set_halo(halo_dict)

    def set_hod(self, hod_dict=None, values=None):
        """simulation_design.py:195-211."""
        if hod_dict is None:
            hod_dict = self._default_param_dict['hod_dict']
        for key in self.params.keys():
            if key in hod_dict and key in values:
                hod_dict[key] = values[key]
        self._input_object.set_hod(hod_dict)

    def write(self, output_name):
        """simulation_design.py:213-220."""
        self.values_frame.to_csv(output_name, index=False, sep=',')


class SimulationDesignFlatUniverse(SimulationDesign):
    """simulation_design.py:223-241: omega_l0 = 1 - omega_m0 - omega_r0 at every point."""

    def __init__(self, input_chomp_object, method_name, params, n_design=100,
                 independent_var=None, default_param_dict=None):
        SimulationDesign.__init__(self, input_chomp_object, method_name, params,
                                  n_design, independent_var, default_param_dict)
        self.set_cosmology(self._default_param_dict['cosmo_dict'], self.params.xs('center'))

    def set_cosmology(self, cosmo_dict=None, values=None):
        if cosmo_dict is None:
            cosmo_dict = self._default_param_dict['cosmo_dict']
        for key in self.params.keys():
            if key in cosmo_dict and key in values:
                cosmo_dict[key] = values[key]
        cosmo_dict['omega_l0'] = 1.0 - cosmo_dict['omega_m0'] - cosmo_dict['omega_r0']
        self._input_object.set_cosmology(cosmo_dict)


class SimulationDesignHubbleNormalizedDensities(SimulationDesign):
    """simulation_design.py:244-267: parameters omega_mh2 = Omega_m h^2, omega_bh2."""

    def __init__(self, input_chomp_object, method_name, params, n_design=100,
                 independent_var=None, default_param_dict=None):
        SimulationDesign.__init__(self, input_chomp_object, method_name, params,
                                  n_design, independent_var, default_param_dict)
        self._vary_cosmology = True
        self.set_cosmology(self._default_param_dict['cosmo_dict'], self.params.xs('center'))

    def set_cosmology(self, cosmo_dict=None, values=None):
        if cosmo_dict is None:
            cosmo_dict = self._default_param_dict['cosmo_dict']
        for key in self.params.keys():
            if key in cosmo_dict and key in values:
                cosmo_dict[key] = values[key]
        cosmo_dict['omega_m0'] = values['omega_mh2'] / cosmo_dict['h'] ** 2
        cosmo_dict['omega_b0'] = values['omega_bh2'] / cosmo_dict['h'] ** 2
        cosmo_dict['omega_l0'] = 1.0 - cosmo_dict['omega_m0'] - cosmo_dict['omega_r0']
        self._input_object.set_cosmology(cosmo_dict)


class SimulationDesignHODWakeAssumptions(SimulationDesign):
    """simulation_design.py:268-293: the HOD design with M_0 tied to M_min (log_M_0 = log_M_min at
    every point) in a flat universe (omega_l0 = 1 - omega_m0 - omega_r0 whenever the cosmology is
    set).  The reference's methods name variables that do not exist there (`params`,
    `cosmo_dict` inside set_hod); this is what they spell out: the design's values by name into
    the dictionary, the derived parameter, then the object's setter with that dictionary."""

    def __init__(self, input_chomp_object, method_name, params, n_design=100,
                 independent_var=None, default_param_dict=None):
        SimulationDesign.__init__(self, input_chomp_object, method_name, params,
                                  n_design, independent_var, default_param_dict)

    def set_cosmology(self, cosmo_dict=None, values=None):
        if cosmo_dict is None:
            cosmo_dict = self._default_param_dict['cosmo_dict']
        for key in self.params.keys():
            if key in cosmo_dict and key in values:
                cosmo_dict[key] = values[key]
        cosmo_dict['omega_l0'] = 1.0 - cosmo_dict['omega_m0'] - cosmo_dict['omega_r0']
        self._input_object.set_cosmology(cosmo_dict)

    def set_hod(self, hod_dict=None, values=None):
        if hod_dict is None:
            hod_dict = self._default_param_dict['hod_dict']
        for key in self.params.keys():
            if key in hod_dict and key in values:
                hod_dict[key] = values[key]
        hod_dict['log_M_0'] = hod_dict['log_M_min']
        self._input_object.set_hod(hod_dict)
