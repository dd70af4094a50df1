"""CPU tests of PerturbationTheory and MassFunctionSecondOrder (perturbation_spectra.py:36-345,
mass_function.py:365-434): the header, exports and ctypes declarations of the new entry points,
the quirks that need no device, and a numpy restatement of the forms (used by the GPU tests with
the device's own P_lin) checked against the reference's numbers (G23) where no P_lin enters."""
import os
import re

import numpy
import pytest

from conftest import ROOT, load_golden

PT_FORMS = ("Fs2", "Fs2_len", "Fs2_kdiff", "Fs3", "Fs3_parallelogram", "F3", "Fs3_BCGS",
            "bispectrum", "bispectrum_len", "trispectrum", "trispectrum_parallelogram")
NO_POWER = ("Fs2", "Fs2_len", "Fs2_kdiff", "Fs3", "Fs3_parallelogram", "F3", "Fs3_BCGS")


# -- numpy restatement: (value, sum of the absolute terms), vectorised over configurations ------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def r_fs2(k1, k2):
    d = _dot(k1, k2)
    k1a = numpy.sqrt(_dot(k1, k1))
    k2a = numpy.sqrt(_dot(k2, k2))
    small = (k1a < 1e-8) | (k2a < 1e-8)
    with numpy.errstate(all="ignore"):
        rat = d / (k1a * k2a)
        t = (rat / 2.) * (k1a / k2a + k2a / k1a)
        u = (2. / 7.) * rat * rat
        v = 5. / 7. + t + u
        s = 5. / 7. + abs(t) + abs(u)
    return numpy.where(small, 5. / 7., v), numpy.where(small, 5. / 7., s)


def r_fs2_len(k1, k2, z):
    with numpy.errstate(all="ignore"):
        t = (z / 2.) * (k1 / k2 + k2 / k1)
        u = (2. / 7.) * z * z
        small = (k1 < 1e-8) | (k2 < 1e-8)
        return (numpy.where(small, 5. / 7., 5. / 7. + t + u),
                numpy.where(small, 5. / 7., 5. / 7. + abs(t) + abs(u)))


def r_fs2_kdiff(k1, k2, mu):
    with numpy.errstate(all="ignore"):
        x = k1 * k1 + k2 * k2 - 2. * k1 * k2 * mu
        z = (k1 * mu - k2) / x
        return r_fs2_len(numpy.sqrt(x), k2, z)


def r_fs3(k1, k2, k3):
    with numpy.errstate(all="ignore"):
        k1a, k2a, k3a = _dot(k1, k1), _dot(k2, k2), _dot(k3, k3)
        k12a, k23a = _dot(k1 + k2, k1 + k2), _dot(k2 + k3, k2 + k3)
        k123a = _dot(k1 + k2 + k3, k1 + k2 + k3)
        b1 = (1. / 21.) * _dot(k1, k2) * k12a + (1. / 14.) * k2a * _dot(k1, k1 + k2)
        b2 = 7. * k3a * _dot(k1 + k2, k1 + k2 + k3) + _dot(k3, k1 + k2) * k123a
        b3 = (1. / 21.) * _dot(k2, k3) * k23a + (1. / 14.) * k3a * _dot(k2, k2 + k3)
        b4 = _dot(k2, k3) * k23a + 5. * k3a * _dot(k2, k2 + k3)
        c1 = numpy.where(k12a < 1e-8, 0.0, 1. / (3. * k1a * k2a * k3a * k12a))
        c3 = numpy.where(k23a < 1e-8, 0.0,
                         (_dot(k1, k2 + k3) * k123a) / (3. * k1a * k2a * k3a * k23a))
        c4 = _dot(k1, k1 + k2 + k3) / (18. * k1a * k2a * k3a)
        t = (c1 * b1 * b2, c3 * b3, c4 * b4)
        return t[0] + t[1] + t[2], abs(t[0]) + abs(t[1]) + abs(t[2])


def r_fs3_par(k1, k2, mu):
    with numpy.errstate(all="ignore"):
        x = k2 / k1
        y = x * mu - 1.0
        z = 1.0 + x * x - 2.0 * x * mu
        t1 = (1. / 21.) * x * y * ((mu / 3.) + 0.5 * x * y / z)
        t2 = -(mu / 18.) * (mu * z + 5 * x * y)
        return t1 + t2, abs(t1) + abs(t2)


def _alpha(k1, k2):
    with numpy.errstate(all="ignore"):
        k1sq = _dot(k1, k1)
        return numpy.where(k1sq == 0.0, 0.0, _dot(k1 + k2, k1) / k1sq)


def _gamma(k1, k2):
    with numpy.errstate(all="ignore"):
        a, b = _dot(k1, k1), _dot(k2, k2)
        return numpy.where(a * b == 0.0, 0.0, 1 - _dot(k1, k2) ** 2 / (a * b))


def _alpha_s(k1, k2):
    """Sum of the absolute terms of alpha_BCGS: (|k1.k1| + |k2.k1|) / k1.k1."""
    with numpy.errstate(all="ignore"):
        k1sq = _dot(k1, k1)
        return numpy.where(k1sq == 0.0, 0.0, (k1sq + abs(_dot(k2, k1))) / k1sq)


def _gamma_s(k1, k2):
    with numpy.errstate(all="ignore"):
        a, b = _dot(k1, k1), _dot(k2, k2)
        return numpy.where(a * b == 0.0, 0.0, 1 + _dot(k1, k2) ** 2 / (a * b))


def _f3_terms(k1, k2, k3, al, ga):
    k12 = k1 + k2
    g312, g12 = ga(k3, k12), ga(k1, k2)
    a3, a12, a1 = al(k3, k12), al(k12, k3), al(k1, k2)
    R11 = (0.5 * a3 + 0.5 * a12 - (1. / 3.) * g312) * a1
    R12 = (-1.5 * a12 - (4. / 3.) * a3 + 2.5 * g312) * g12
    R2 = 0.75 * (a3 + a12 - 3. * g312) * g12
    R3 = (3. / 8.) * g312 * g12
    R4 = (2. / 3.) * g312 * a1 - ((1. / 3.) * a3 + 0.5 * g312) * g12
    return R11, R12, R2, R3, R4


def r_f3(k1, k2, k3):
    R11, R12, R2, R3, R4 = _f3_terms(k1, k2, k3, _alpha, _gamma)
    # the scale: every term with alpha and gamma replaced by the sums of their absolute terms
    S = _f3_terms(k1, k2, k3, _alpha_s, _gamma_s)
    scale = 0.0
    for c, x in zip((1.0, 1.0, 34. / 21., 682. / 189., 9. / 10.), S):
        scale = scale + c * (abs(x) + 5.0 * _alpha_s(k1, k2) * (1 + _gamma_s(k1, k2)) *
                             (_alpha_s(k3, k1 + k2) + _alpha_s(k1 + k2, k3) +
                              _gamma_s(k3, k1 + k2)))
    return ((R11 + R12) + (34. / 21.) * R2 + (682. / 189.) * R3 + (9. / 10.) * R4), scale


def r_fs3_bcgs(k1, k2, k3):
    parts = [r_f3(*p) for p in ((k1, k2, k3), (k3, k1, k2), (k2, k3, k1), (k2, k1, k3),
                                (k3, k2, k1), (k1, k3, k2))]
    v = parts[0][0]
    for p in parts[1:]:
        v = v + p[0]
    return v / 6., sum(p[1] for p in parts) / 6.


def r_bispectrum(P, k1, k2, k3):
    p1, p2, p3 = (P(numpy.sqrt(_dot(k, k))) for k in (k1, k2, k3))
    t = (r_fs2(k1, k2)[0] * p1 * p2, r_fs2(k1, k3)[0] * p1 * p3, r_fs2(k2, k3)[0] * p2 * p3)
    return 2. * (t[0] + t[1] + t[2]), 2. * sum(abs(x) for x in t)


def r_bispectrum_len(P, k1, k2, k3, z12, z13, z23):
    p1, p2, p3 = P(k1), P(k2), P(k3)
    t = (r_fs2_len(k1, k2, z12)[0] * p1 * p2, r_fs2_len(k1, k3, z13)[0] * p1 * p3,
         r_fs2_len(k2, k3, z23)[0] * p2 * p3)
    return 2. * (t[0] + t[1] + t[2]), 2. * sum(abs(x) for x in t)


def r_trispectrum(P, k1, k2, k3, k4):
    def pl(k):
        return P(numpy.sqrt(_dot(k, k)))
    p1, p2, p3, p4 = pl(k1), pl(k2), pl(k3), pl(k4)
    p12, p13, p14 = pl(k1 + k2), pl(k1 + k3), pl(k1 + k4)
    p23, p24, p34 = pl(k2 + k3), pl(k2 + k4), pl(k3 + k4)
    p12 = numpy.where(numpy.isnan(p12), 0.0, p12)
    p34 = numpy.where(numpy.isnan(p34), 0.0, p34)

    def f(a, b):
        return r_fs2(a, b)[0]
    t1 = [f(k1 + k2, -k1) * f(k1 + k2, k3) * p1 * p12 * p3,
          f(k2 + k3, -k2) * f(k2 + k3, k1) * p2 * p23 * p1,
          f(k3 + k1, -k3) * f(k3 + k1, k2) * p3 * p13 * p2,
          f(k1 + k2, -k1) * f(k1 + k2, k4) * p1 * p12 * p4,
          f(k2 + k4, -k2) * f(k2 + k4, k1) * p2 * p24 * p1,
          f(k4 + k1, -k4) * f(k4 + k1, k2) * p4 * p14 * p2,
          f(k1 + k3, -k1) * f(k1 + k3, k4) * p1 * p13 * p4,
          f(k3 + k4, -k3) * f(k3 + k4, k1) * p3 * p34 * p1,
          f(k4 + k1, -k4) * f(k4 + k1, k3) * p4 * p14 * p3,
          f(k2 + k3, -k2) * f(k2 + k3, k4) * p2 * p23 * p4,
          f(k3 + k4, -k3) * f(k3 + k4, k2) * p3 * p34 * p2,
          f(k4 + k2, -k4) * f(k4 + k2, k3) * p4 * p24 * p3]
    t2 = [r_fs3(k1, k2, k3)[0] * p1 * p2 * p3, r_fs3(k1, k2, k4)[0] * p1 * p2 * p4,
          r_fs3(k1, k3, k4)[0] * p1 * p3 * p4, r_fs3(k2, k3, k4)[0] * p2 * p3 * p4]
    b1 = t1[0]
    for x in t1[1:]:
        b1 = b1 + x
    b2 = t2[0]
    for x in t2[1:]:
        b2 = b2 + x
    return 4. * b1 + 6. * b2, 4. * sum(abs(x) for x in t1) + 6. * sum(abs(x) for x in t2)


def r_trispectrum_par(P, k1, k2, mu):
    with numpy.errstate(all="ignore"):
        x = k2 / k1
        z = 1 + x ** 2 - 2 * x * mu
        p1, p2, p12 = P(k1), P(k2), P(k1 * numpy.sqrt(z))
        F21, F22 = r_fs2_kdiff(k1, k2, mu)[0], r_fs2_kdiff(k2, k1, mu)[0]
        a1 = 12. * r_fs3_par(k1, k2, mu)[0] * (p1 ** 2) * p2
        a2 = 8. * F21 ** 2 * p12 * p2 ** 2
        a3 = 16. * F21 * F22 * p1 * p2 * p12
        b1 = 12. * r_fs3_par(k2, k1, mu)[0] * (p2 ** 2) * p1
        b2 = 8. * F22 ** 2 * p12 * p1 ** 2
        t = (a1, b1, a2, b2, 2. * a3)
        return a1 + b1 + a2 + b2 + 2. * a3, sum(abs(v) for v in t)


def restate(form, args, P=None):
    """The form on configurations args [N, arity]: (value, sum of the absolute terms)."""
    a = numpy.asarray(args, dtype=numpy.float64)
    vec = [a[:, 3 * j:3 * j + 3] for j in range(a.shape[1] // 3)]
    col = [a[:, j] for j in range(a.shape[1])]
    if form == "Fs2":
        return r_fs2(*vec)
    if form == "Fs2_len":
        return r_fs2_len(*col)
    if form == "Fs2_kdiff":
        return r_fs2_kdiff(*col)
    if form == "Fs3":
        return r_fs3(*vec)
    if form == "Fs3_parallelogram":
        return r_fs3_par(*col)
    if form == "F3":
        return r_f3(*vec)
    if form == "Fs3_BCGS":
        return r_fs3_bcgs(*vec)
    if form == "bispectrum":
        return r_bispectrum(P, *vec)
    if form == "bispectrum_len":
        return r_bispectrum_len(P, *col)
    if form == "trispectrum":
        return r_trispectrum(P, *vec)
    return r_trispectrum_par(P, *col)


def close_or_same(got, want, scale, tol):
    """Finite values within tol of the sum of the absolute terms; inf / NaN in the same places."""
    got, want, scale = (numpy.asarray(x, dtype=float) for x in (got, want, scale))
    fin = numpy.isfinite(want)
    assert numpy.array_equal(numpy.isfinite(got), fin)
    assert numpy.array_equal(numpy.isnan(got), numpy.isnan(want))
    assert numpy.array_equal(got[numpy.isinf(want)], want[numpy.isinf(want)])
    err = numpy.abs(got[fin] - want[fin]) / numpy.maximum(scale[fin], 1e-300)
    assert err.size == 0 or err.max() < tol, err.max()


# -- tests ---------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "chomp_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_new_entries():
    text = _declared()
    for name in ("chomp_pt_eval", "chomp_set_second_order", "chomp_get_second_order"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
    from chomp_amd import _lib
    for name in ("chomp_pt_eval", "chomp_set_second_order", "chomp_get_second_order"):
        assert name in _lib.EXPORTS
    defines = dict(re.findall(r"#define (CHOMP_\w+) (\S+)", text))
    for form, i in _lib.PT.items():
        assert int(defines["CHOMP_PT_" + form.upper()]) == i, form
    assert sorted(_lib.PT) == sorted(PT_FORMS)
    assert int(defines["CHOMP_EV_BIAS_2_NU"]) == _lib.EV["bias_2_nu"]
    assert int(defines["CHOMP_EV_SIGMA_OF_NU"]) == _lib.EV["sigma_of_nu"]
    assert int(defines["CHOMP_ST_B2_DIVMAX"].rstrip("u"), 16) == _lib.ST_B2_DIVMAX


def test_ctypes_declarations():
    import ctypes
    from chomp_amd import _lib
    L = _lib.lib()
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert L.chomp_pt_eval.argtypes == [vp, i, sz, sz, vp, sz, vp, i]
    assert L.chomp_set_second_order.argtypes == [vp, i]
    assert L.chomp_get_second_order.argtypes == [vp, sz, _lib.c_double_p, sz]
    for name in ("chomp_pt_eval", "chomp_set_second_order", "chomp_get_second_order"):
        assert getattr(L, name).restype == i
    assert _lib.PT_ARITY == {"Fs2": 6, "Fs2_len": 3, "Fs2_kdiff": 3, "Fs3": 9,
                             "Fs3_parallelogram": 3, "F3": 9, "Fs3_BCGS": 9, "bispectrum": 9,
                             "bispectrum_len": 6, "trispectrum": 12,
                             "trispectrum_parallelogram": 3}
    assert "B2" in "".join(_lib.describe_status(_lib.ST_B2_DIVMAX)).upper() or \
        "bias_2_norm" in _lib.describe_status(_lib.ST_B2_DIVMAX)[0]


def test_package_exports_perturbation_spectra():
    import chomp_amd
    assert "perturbation_spectra" in chomp_amd.__all__
    ps = chomp_amd.perturbation_spectra
    for name in PT_FORMS + ("bispectrum_many", "trispectrum_many", "set_cosmology",
                            "set_cosmology_object", "set_redshift"):
        assert callable(getattr(ps.PerturbationTheory, name)), name
    from chomp_amd import _lib, mass_function
    mf = mass_function.MassFunctionSecondOrder
    assert issubclass(mf, mass_function.MassFunction) and mf._kind == _lib.MF_ST
    for name in ("bias_2_nu", "bias_2_mass", "_sigma_spline"):
        assert callable(getattr(mf, name))


def test_set_redshift_raises_as_shipped():
    from chomp_amd import cosmology, perturbation_spectra
    g = load_golden("g23_perturbation")
    e = cosmology.SingleEpoch(0.0)
    pt = perturbation_spectra.PerturbationTheory(0.5, e)
    assert e._redshift == 0.5 == float(g["quirk_moved_redshift"])   # the caller's object moved
    assert int(g["quirk_set_redshift_raises"]) == 1
    with pytest.raises(AttributeError, match="set_redshif'"):
        pt.set_redshift(1.0)
    assert pt._redshift == 1.0 == float(g["quirk_redshift_after"])
    assert e._redshift == 0.5


def test_fs3_bcgs_with_a_callable_is_out_of_scope():
    from chomp_amd import _lib, cosmology, perturbation_spectra
    pt = perturbation_spectra.PerturbationTheory(0.0, cosmology.SingleEpoch(0.0))
    k = numpy.array([0.1, 0.0, 0.0])
    with pytest.raises(_lib.ChompScopeError):
        pt.Fs3_BCGS(k, k, k, F3=lambda a, b, c: 1.0)
    with pytest.raises(ValueError):
        pt.Fs2(numpy.ones((2, 3)), numpy.ones((2, 3)))


def test_alpha_gamma_zero_on_exact_zeros():
    from chomp_amd.perturbation_spectra import alpha_BCGS, gamma_BCGS
    z, k = numpy.zeros(3), numpy.array([0.1, 0.2, -0.3])
    assert alpha_BCGS(z, k) == 0.0 and gamma_BCGS(z, k) == 0.0 and gamma_BCGS(k, z) == 0.0
    assert alpha_BCGS(k, k) == 2.0
    assert gamma_BCGS(k, 2 * k) == pytest.approx(0.0, abs=1e-15)


@pytest.mark.parametrize("form", NO_POWER)
def test_restatement_matches_reference(form):
    g = load_golden("g23_perturbation")
    args = g["pt_args_" + form]
    v, s = restate(form, args)
    for zt in ("def_z000_", "def_z050_", "c2_z000_", "c2_z050_"):
        close_or_same(v, g[zt + form], s, 1e-12)


def test_fs3_and_fs3_bcgs_disagree_as_shipped():
    g = load_golden("g23_perturbation")
    a = g["def_z000_Fs3"][:256]
    b = g["def_z000_Fs3_BCGS"][:256]
    assert numpy.abs(a - b).max() > 1e-3 * numpy.abs(a).max()
