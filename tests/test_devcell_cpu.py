"""tests/devcell_ref.py checked without a GPU: the plan of the C_l work buffer restated in Python
is the header's own (through the harness's host getters: hipcc cross-compiles, nothing is
launched), the projection set-ups test_gpu_devcell.py hands in reach every range rule they
advertise with no decision near its threshold, the restatement of the node table agrees with a
plain fp64 evaluation of the same coefficients within its own bound, and the spline families are
what the long-double solve and FITPACK agree on."""
import ctypes

import numpy
import pytest
from scipy.interpolate import InterpolatedUnivariateSpline

import devcheck_build
import devcell_ref as c
from devcell_ref import LD

needs_hipcc = pytest.mark.skipif(not devcheck_build.have_hipcc(), reason="hipcc is not installed")

DIVMAX = (5, 6, 8, 11, 12, 16, 17, 20, 22)
NS = (1, 15, 16, 511, 513, 2048)


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(devcheck_build.build(harness="devcell"))
    for name, argtypes in devcheck_build.CELL_ENTRY_POINTS.items():
        getattr(L, name).argtypes = argtypes
    return L


@needs_hipcc
def test_plan_is_the_headers(lib):
    """cell_plan, cell_epoch_stride, cell_set_stride and make_proj_layout: every field, exactly,
    over divmax, n, both layouts, one_kernel and per_row_nodes; and what the fields promise."""
    k = (ctypes.c_int * 5)()
    lib.dl_constants(k)
    assert list(k) == [c.CELL_TAB_LEVEL, c.CELL_SPLIT_LEVEL, c.CELL4_LEVEL, c.DEEP_THREADS, c.DEEP_LDS]
    assert lib.dl_romberg_dump() == c.ROMBERG_DUMP and lib.dl_ptab_n() == c.PTAB_N
    lay = (ctypes.c_int * 7)()
    for NC, NWp in ((8, 8), (50, 100)):
        assert lib.dl_proj_layout(NC, NWp, c.NKT, lay) == 0
        L = c.proj_layout(NC, NWp)
        assert list(lay) == [L["me_chi0"], L["me_pp_z0"], L["me_pp_g0"], L["w_pp0"], L["w_pp1"],
                             L["total"], L["lds"]]
    assert lib.dl_proj_layout(3, 8, c.NKT, lay) == -1
    out = (ctypes.c_longlong * 20)()
    seen = set()
    for divmax in DIVMAX:
        for n in NS:
            for one in (0, 1):
                for rows in (0, 1):
                    for NK, NC, NWp in ((8, 8, 8), (50, 50, 100)):
                        assert lib.dl_plan(divmax, NK, NC, NWp, c.NKT, n, one, rows, out) == 0
                        want = c.plan(divmax, NK, NC, NWp, n, one, rows)
                        assert list(out) == want, (divmax, n, one, rows, NK)
                        P = dict(zip(c.PLAN_FIELDS, want))
                        # the list (ints) starts on a double (deep_at counts doubles: 8-byte
                        # aligned), right behind the n states
                        assert isinstance(P["deep_at"], int) and P["deep_at"] == P["state_at"] + 34 * n
                        # a slab holds its spectrum table, n states and 2 + n ints
                        assert P["stride"] - (P["deep_at"] - (0 if rows else P["pk_at"])) >= (n + 3) // 2
                        assert P["stride"] - (P["deep_at"] - (0 if rows else P["pk_at"])) <= (n + 3) // 2 + 1
                        assert P["LT"] == min(divmax, 16) and P["gdeep"] == min(n, 512)
                        assert P["split"] == (divmax if one or divmax <= 11 else 11)
                        assert P["four"] == int(P["split"] >= 6 and P["split"] <= P["LT"] and n >= 16)
                        assert P["deep_fits"] == 1
                        seen.add((P["four"], P["split"] < divmax, P["LT"] < divmax))
    # both kernels, with and without a hand-over, with and without levels beyond the table
    assert {(1, True, True), (1, True, False), (1, False, False), (0, False, False),
            (0, True, True), (0, False, True)} <= seen
    assert lib.dl_plan(12, 2000, 50, 100, c.NKT, 16, 0, 0, out) == 0 and out[4] == 0   # (too large)


def test_projection_cases_reach_their_rules():
    """From the reference alone: every window rule -- a range equal to [chi_min, chi_max], strictly
    inside it, overhanging it on either side, and one so narrow that nodes 0, 1 and the midpoint
    all see zero -- and growth_factor's "1 outside" rule are taken at the levels the GPU test runs,
    and no node's redshift lies within 1e-9 of the end of the growth table (the one discontinuous
    decision)."""
    P = c.proj_cases()
    a, b = P["equal"].chi_min, P["equal"].chi_max
    assert P["equal"].wr == [(a, b), (a, b)]
    assert all(a < lo and hi < b for lo, hi in P["inside"].wr)
    assert P["overhang"].wr[0][0] < a and P["overhang"].wr[1][0] < a and P["overhang"].wr[1][1] > b
    assert P["overhang"].F(numpy.array([a]), 0.77)[0][0] > 0       # (not zero at the lower end)
    for name, LT in (("equal", 6), ("inside", 9), ("overhang", 9), ("narrow", 6), ("growth_ends", 9),
                     ("overhang", 16), ("growth_ends", 16)):
        chi = c.node_chi(P[name].chi_min, P[name].chi_max, LT)[0].astype(float)
        F, bound, (both, ig, z) = P[name].F(chi, 0.77)
        assert numpy.min(numpy.abs(z - LD(P[name].z_hi))) > 1e-9, name
        assert numpy.min(numpy.abs(z - LD(P[name].z_lo))) > 1e-9, name
        assert numpy.all(F[~both] == 0), name
        if name == "equal":
            assert both.all() and F[0] == 0 and abs(F[1]) <= bound[1]     # (the bump ends at 0)
        if name in ("inside", "overhang"):
            assert (~both).sum() > 8 and both.sum() > 8
        if name == "narrow":
            assert numpy.all(F[:3] == 0) and both.sum() >= 8
        if name == "growth_ends":
            assert (~ig).sum() > 8 and ig.sum() > 8 and numpy.any(~ig & (F != 0))
        else:
            assert ig.all()
        # a plain fp64 evaluation of the same coefficients lies within the bound, and the bound
        # is a rounding bound: below 1e-13 of the largest |F|
        z64 = c.pp_eval(P[name].chi_k, P[name].pp_z, chi).astype(float)
        ins = (z64 <= P[name].z_hi) & (z64 >= P[name].z_lo)
        zk = numpy.linspace(P[name].z_lo, P[name].z_hi, P[name].NC)
        D = numpy.where(ins, c.pp_eval(zk, P[name].pp_g, z64).astype(float), 1.0)
        w = [numpy.where((chi >= lo) & (chi <= hi),
                         c.pp_eval(P[name].w_x[i], P[name].pp_w[i], chi).astype(float), 0.0)
             for i, (lo, hi) in enumerate(P[name].wr)]
        plain = (1.0 / (0.77 * 0.77)) * w[0] * w[1] * D * D / (chi * chi)
        assert numpy.all(numpy.abs(plain.astype(LD) - F) <= bound), name
        assert float(numpy.max(bound)) < 1e-13 * float(numpy.max(numpy.abs(F))), name


def test_node_index_map():
    """idx = 1 + 2^(lev - 1) + j, idx 0 -> a, idx 1 -> b: a bijection onto 0 .. 2^LT, the nodes
    of level lev the odd multiples of (b - a) / 2^lev."""
    a, b = 400.0, 2600.0
    chi, lev, j = c.node_chi(a, b, 6)
    assert [c.node_index(int(l), int(q)) for l, q in zip(lev, j)] == list(range(65))
    grid = numpy.sort(chi.astype(float))
    assert numpy.allclose(grid, numpy.linspace(a, b, 65), rtol=1e-15)
    for l in range(1, 7):
        x = chi[lev == l].astype(float)
        m = (x - a) / (b - a) * 2 ** l
        assert numpy.allclose(m, numpy.arange(1, 2 ** l, 2), rtol=1e-14)


@pytest.mark.parametrize("name", c.FAMILIES)
def test_spline_families(name):
    """Every knot family at the sizes the GPU test builds: strictly increasing knots, finite
    values, and the long-double not-a-knot solve is the spline FITPACK builds (1e-9 of the table's
    scale: the cross-check of the restatement, far above either's rounding)."""
    for n in (4, 5, 50, 65, 128):
        x, y = c.family(name, n)
        assert x.size == y.size == n and numpy.all(numpy.diff(x) > 0) and numpy.isfinite(y).all()
        pp = c.nak_pp(x, y)
        xe = numpy.linspace(x[0], x[-1], 500)
        fit = InterpolatedUnivariateSpline(x, y, k=3)(xe)
        err = float(numpy.max(numpy.abs(c.pp_eval(x, pp, xe) - fit))) / float(numpy.max(numpy.abs(y)))
        print("%s n %d: long double against FITPACK %.3g" % (name, n, err))
        assert err < 1e-9, (name, n)


# -------------------------------------------------------------------------------------------
# the C_l launches: the value pins the level, and the launches cover what they advertise
# -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references():
    """Per launch: (case, fields, the full reference and the reference up to `split` of every
    multipole), on the reference's own stand-ins for the tables the kernels read."""
    P = c.proj_cases()
    out = {}
    for name in c.LAUNCHES:
        case, L = c.launch(name, projs=P)
        T = c.Tables.host(case)
        full = [case.reference(T, il) for il in range(case.ell.size)]
        first = [case.reference(T, il, upto=case.split) for il in range(case.ell.size)]
        out[name] = (case, L, full, first)
    for form, name in c.ROW_RUNS:                                 # the rows of the batched forms
        for y in range(3):
            case, L = c.row_case(form, name, y, projs=P)
            T = c.Tables.host(case)
            out[case.name] = (case, L, [case.reference(T, il) for il in range(case.ell.size)],
                              [case.reference(T, il, upto=case.split) for il in range(case.ell.size)])
    return out


def test_the_value_pins_the_level(references):
    """(a) and (b) of devcell_ref.pins_the_level for EVERY multipole of every launch, for the whole
    integral and for the part up to `split` (what the first kernel returns)."""
    tightest = [numpy.inf, numpy.inf]
    for name, (case, L, full, first) in references.items():
        for il in range(case.ell.size):
            for ref in (full[il], first[il]):
                a_ok, b_ok = c.pins_the_level(ref)
                assert a_ok and b_ok, (name, il, case.ell[il], ref["level"], a_ok, b_ok)
                if ref["value"] != 0:
                    rel = ref["bound"] / abs(float(ref["value"]))
                    s = ref["level"]
                    tightest[0] = min([tightest[0]] + [abs(m - 1.0) / rel for m in ref["margins"][:s]])
                    tightest[1] = min(tightest[1], float(abs(ref["rows"][s] - ref["rows"][s - 1])) / ref["bound"])
    print("closest decision: %.3g bounds from its threshold (asked: 1e3); closest neighbouring rows: "
          "%.3g bounds apart (asked: 8)" % tuple(tightest))


def test_launches_cover_what_they_advertise(references):
    levels, kinds, unfinished = {}, set(), {}
    fast_fails = False
    for name, (case, L, full, first) in references.items():
        assert case.ell.size == L["n"] <= 48 and L["LT"] <= 12 and L["divmax"] <= 12
        for il, ref in enumerate(full):
            key = ("exhausted" if not ref["converged"] else
                   "beyond" if ref["level"] > L["LT"] else ref["level"])
            levels.setdefault(key, []).append((name, il))
            kinds |= ref["kinds"]
            fast_fails |= ref["fast_fails"]
            if ref["level"] == 1 and ref["converged"] and ref["value"] == 0:
                levels.setdefault("zero", []).append((name, il))
        unfinished[name] = sum(not f["converged"] for f in first)
        if L["split"] < L["divmax"]:
            assert unfinished[name] >= 1, name                    # someone is handed over
    print({k: len(v) for k, v in levels.items()}, unfinished)
    assert "zero" in levels and "beyond" in levels and "exhausted" in levels
    assert any(k in levels for k in (2, 3, 4, 5)) and 6 in levels
    assert any(k in levels for k in (7, 8)) and any(k in levels for k in (9, 10, 11)) and 12 in levels
    assert kinds == {c.STENCIL, c.ZERO, c.AT_LN, c.DIRECT, c.AT_LN_HF, c.AT_LN_TAIL}
    # at_ln's HaloFit P_mm on both sides of the range and the extrapolate tail, inside the table,
    # among the multipoles handed on to k_cell_deep, in a batch of four with a refusal
    for name, kind in (("hf_mm_hand", c.AT_LN_HF), ("ext_hand", c.AT_LN_TAIL)):
        case, L, full, first = references[name]
        deep = [f for f, g in zip(full, first) if not g["converged"]]
        assert any(kind in f["kinds"] and f["fast_fails"] for f in deep), name
    case = references["hf_mm_hand"][0]
    k = case.ell[:, None] / numpy.array([case.proj.chi_min, case.proj.chi_max])[None, :]
    assert (k < 1e-3).any() and (k > 1e2).any()
    assert fast_fails                     # a k_cell_deep batch with one of its four nodes refused
    # a list of >= 7 drawn by 1 and by 3 blocks; the n_ell of k_cell4's last block; every split
    assert unfinished["four_8"] >= 7 and c.LAUNCHES["four_8"][-1] == 1
    assert unfinished["cell_hand"] >= 7 and c.LAUNCHES["cell_hand"][-1] == 3
    four = [v for v in c.LAUNCHES.values() if v[10] == c.K_FOUR]
    assert {v[5] for v in four} == {16, 17, 18, 19, 40} and {v[9] for v in four} == {6, 8, 11}
    assert {v[9] < v[7] for v in four} == {True, False}


def test_replay_is_the_oracles_romberg():
    """The rows replayed in long double stop where oracle/romberg.py (scipy's rule) stops on the
    same node values, with the same value to fp64 rounding."""
    from oracle import romberg as orom
    case, L = c.launch("cell_direct")
    T = c.Tables.host(case)
    for il in (4, 20, 27, 28, 31, 33):
        ref = case.reference(T, il)
        seen = {}

        def f(x):
            if numpy.isscalar(x):
                return float(case.level_nodes(T, il, 0)[0][0 if x == case.proj.chi_min else 1])
            lev = int(numpy.log2(x.size)) + 1
            seen[lev] = x
            return case.level_nodes(T, il, lev)[0].astype(float)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            v, lev = orom.romberg(f, case.proj.chi_min, case.proj.chi_max, tol=c.TOL, rtol=case.rtol,
                                  divmax=case.divmax, vec_func=True, return_level=True)
        assert lev == ref["level"], (il, lev, ref["level"])
        assert abs(v - float(ref["value"])) <= 1e-12 * abs(v) + 1e-300
        # the rule's own nodes are the table's under the index map
        for q, x in seen.items():
            if q <= T.LT:
                idx = 1 + (1 << (q - 1)) + numpy.arange(1 << (q - 1))
                assert numpy.max(numpy.abs(x - T.chi[idx]) / c.ulp(x)) <= 1.0
