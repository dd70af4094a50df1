"""The device harnesses (tests/devcheck: devcheck.hip, the fp64 primitives and the wavefront
Romberg; devphys.hip, the halo-model physics; devproj.hip, the moment route of w(theta), the
bicubic tables and the quintic derivatives; devpower.hip, the spectrum evaluator and the Stage E
launch shapes; devcell.hip, the C_l route and the parallel spline build) compile for
gfx950 against the current headers and export every entry point the GPU tests
(test_gpu_devmath.py, test_gpu_romberg.py; test_gpu_devphys.py; test_gpu_devproj.py;
test_gpu_devpower.py; test_gpu_devcell.py) use.  No GPU is needed: hipcc cross-compiles.  This
keeps the harness from rotting when a header's signature changes in a change developed without
a GPU."""
import ctypes
import os
import re

import pytest

import devcheck_build


@pytest.mark.skipif(not devcheck_build.have_hipcc(), reason="hipcc is not installed")
def test_devcheck_compiles_and_exports():
    path = devcheck_build.build()
    assert devcheck_build.build() == path                     # (second call: nothing to do)
    with open(devcheck_build.HASH) as f:
        assert f.read().strip() == devcheck_build.source_hash()
    L = ctypes.CDLL(path)
    for name in devcheck_build.ENTRY_POINTS:
        assert hasattr(L, name), name
    # the getters run on the host
    L.dc_case_stride.restype = ctypes.c_int
    assert L.dc_case_stride() == 16 and L.dc_out_stride() == 8
    assert L.dc_index_out_stride() == 3 * 34 + 2
    assert L.dc_fma_k_count() == 6
    # the flags are the product's, not a copy
    from chomp_amd import _lib
    assert devcheck_build.flags() == _lib.HIPCC_FLAGS + _lib.NO_LICM


@pytest.mark.skipif(not devcheck_build.have_hipcc(), reason="hipcc is not installed")
def test_devphys_compiles_and_exports():
    H = devcheck_build.HARNESSES["devphys"]
    other = devcheck_build.HARNESSES["devcheck"]
    devcheck_build.build()
    stamp = os.stat(other.so).st_mtime_ns
    path = devcheck_build.build(harness="devphys")
    assert path == H.so != other.so
    assert devcheck_build.build(harness="devphys") == path
    assert os.stat(other.so).st_mtime_ns == stamp             # (the other harness: left alone)
    with open(H.hash) as f:
        assert f.read().strip() == devcheck_build.source_hash("devphys")
    L = ctypes.CDLL(path)
    for name in devcheck_build.PHYS_ENTRY_POINTS:
        assert hasattr(L, name), name
    # every entry point the GPU tests name is declared (and so exported, above)
    here = os.path.dirname(os.path.abspath(__file__))
    for test in ("test_gpu_devphys.py",):
        with open(os.path.join(here, test)) as f:
            named = set(re.findall(r"\b(dp_[a-z0-9_]+)\b", f.read()))
        assert named, test
        assert named <= set(devcheck_build.PHYS_ENTRY_POINTS), named
    # the getters run on the host
    L.dp_sizeof_epoch.restype = ctypes.c_int
    L.dp_epoch_field_names.restype = ctypes.c_char_p
    names = L.dp_epoch_field_names().decode().strip(",").split(",")
    raw = (ctypes.c_int * (2 * len(names)))()
    L.dp_epoch_offsets(raw)
    size = L.dp_sizeof_epoch()
    assert size % 16 == 0 and names[0] == "om0" and raw[0] == 0
    assert all(0 <= raw[2 * j] <= size - (4 if raw[2 * j + 1] else 8) for j in range(len(names)))
    assert len(set(raw[0::2])) == len(names)
    assert raw[2 * names.index("mf_kind") + 1] == 1 and raw[2 * names.index("delta_c") + 1] == 0


@pytest.mark.skipif(not devcheck_build.have_hipcc(), reason="hipcc is not installed")
def test_devproj_compiles_and_exports():
    H = devcheck_build.HARNESSES["devproj"]
    others = [devcheck_build.HARNESSES[n] for n in ("devcheck", "devphys")]
    devcheck_build.build()
    devcheck_build.build(harness="devphys")
    stamps = [os.stat(o.so).st_mtime_ns for o in others]
    path = devcheck_build.build(harness="devproj")
    assert path == H.so and all(path != o.so for o in others)
    stamp = os.stat(path).st_mtime_ns
    assert devcheck_build.build(harness="devproj") == path
    assert os.stat(path).st_mtime_ns == stamp                 # (second call: nothing to do)
    assert [os.stat(o.so).st_mtime_ns for o in others] == stamps   # (the others: left alone)
    with open(H.hash) as f:
        assert f.read().strip() == devcheck_build.source_hash("devproj")
    L = ctypes.CDLL(path)
    for name in devcheck_build.PROJ_ENTRY_POINTS:
        assert hasattr(L, name), name
    assert set(devcheck_build.VOID["devproj"]) <= set(devcheck_build.PROJ_ENTRY_POINTS)
    assert devcheck_build.ALL_ENTRY_POINTS["devproj"] is devcheck_build.PROJ_ENTRY_POINTS
    # a prefix of its own: no name of another harness's
    assert all(n.startswith("dj_") for n in devcheck_build.PROJ_ENTRY_POINTS)
    # every entry point the GPU tests name is declared (and so exported, above)
    here = os.path.dirname(os.path.abspath(__file__))
    for test in ("test_gpu_devproj.py",):
        with open(os.path.join(here, test)) as f:
            named = set(re.findall(r"\b(dj_[a-z0-9_]+)\b", f.read()))
        assert named, test
        assert named <= set(devcheck_build.PROJ_ENTRY_POINTS), named
    # the getters run on the host: the constants and sizes of chomp_proj_kernels.h
    assert L.dj_wth_items() == 8 and L.dj_wth_parts() == 8
    L.dj_wth_sizes.argtypes = [ctypes.c_int] * 3 + [devcheck_build.c_double_p]
    out = (ctypes.c_double * 4)()
    assert L.dj_wth_sizes(3, 5, 0, out) == 0
    n_nodes, n_rec, n_tot = 9, 4 * (8 // 8 + 2), 4 * 4 * 5
    assert list(out) == [n_nodes + 1 + n_rec + n_tot + 2, n_nodes + 1, n_nodes + 1 + n_rec, 0]
    assert L.dj_wth_sizes(3, 5, 2, out) == 0
    assert out[3] % 2 == 0 and out[3] >= n_nodes + 1 + n_rec + n_tot + 2 and out[0] == 2 * out[3]
    assert L.dj_wth_sizes(21, 5, 0, out) == -1                # (beyond the node table's level)
    x = (ctypes.c_double * 7)()
    L.dj_quintic_grid.argtypes = [ctypes.c_int, devcheck_build.c_double_p]
    L.dj_quintic_grid.restype = None
    L.dj_quintic_grid(7, x)
    import math
    assert x[0] == math.log(0.1) and x[6] == math.log(10.0) and list(x) == sorted(x)


@pytest.mark.skipif(not devcheck_build.have_hipcc(), reason="hipcc is not installed")
def test_devpower_compiles_and_exports():
    H = devcheck_build.HARNESSES["devpower"]
    others = [devcheck_build.HARNESSES[n] for n in ("devcheck", "devphys", "devproj")]
    for o in others:
        devcheck_build.build(harness=o.name)
    stamps = [os.stat(o.so).st_mtime_ns for o in others]
    path = devcheck_build.build(harness="devpower")
    assert path == H.so and all(path != o.so for o in others)
    stamp = os.stat(path).st_mtime_ns
    assert devcheck_build.build(harness="devpower") == path
    assert os.stat(path).st_mtime_ns == stamp                 # (second call: nothing to do)
    assert [os.stat(o.so).st_mtime_ns for o in others] == stamps   # (the others: left alone)
    with open(H.hash) as f:
        assert f.read().strip() == devcheck_build.source_hash("devpower")
    L = ctypes.CDLL(path)
    for name in devcheck_build.POWER_ENTRY_POINTS:
        assert hasattr(L, name), name
    assert set(devcheck_build.VOID["devpower"]) <= set(devcheck_build.POWER_ENTRY_POINTS)
    assert devcheck_build.ALL_ENTRY_POINTS["devpower"] is devcheck_build.POWER_ENTRY_POINTS
    assert all(n.startswith("dw_") for n in devcheck_build.POWER_ENTRY_POINTS)
    # every entry point the GPU test names is declared (and so exported, above)
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "test_gpu_devpower.py")) as f:
        named = set(re.findall(r"\b(dw_[a-z0-9_]+)\b", f.read()))
    assert named and named <= set(devcheck_build.POWER_ENTRY_POINTS), named
    # the package never loads it
    from chomp_amd import _lib
    assert not any("devpower" in src for src, _ in _lib.UNITS)
    # its hash covers the header chain and the epoch filler it shares with devphys.hip
    for name in ("devpower", "devphys"):
        base = [os.path.basename(p) for p in devcheck_build.HARNESSES[name].headers]
        assert "epoch_fill.h" in base, name
    base = [os.path.basename(p) for p in H.headers]
    for need in ("chomp_cov_kernels.h", "chomp_proj_kernels.h", "chomp_power_kernels.h",
                 "chomp_halo_kernels.h", "chomp_mass_kernels.h", "chomp_romberg.h",
                 "chomp_math.h", "special_tables.h", "chomp_mi355x.h"):
        assert need in base, need
    # the getters run on the host: the constants of the headers
    with open(os.path.join(_lib.CSRC, "chomp_proj_kernels.h")) as f:
        n_tab = int(re.search(r"constexpr int kPTabN = (\d+);", f.read()).group(1))
    with open(os.path.join(_lib.CSRC, "chomp_power_kernels.h")) as f:
        m = re.search(r"kWaveIdxMask = (\w+), kWaveSlow = 1 << (\d+), kWaveTwo = 1 << (\d+);", f.read())
    assert L.dw_ptab_n() == n_tab == 8192
    bits = (ctypes.c_int * 3)()
    L.dw_wave_bits(bits)
    assert list(bits) == [int(m.group(1), 0), 1 << int(m.group(2)), 1 << int(m.group(3))]
    P = devcheck_build.HARNESSES["devphys"]
    Lp = ctypes.CDLL(P.so)
    assert L.dw_sizeof_epoch() == Lp.dp_sizeof_epoch() and L.dw_sizeof_epoch() % 16 == 0
    assert L.dw_epoch_inputs() == Lp.dp_epoch_inputs() + 12
    lay = (ctypes.c_int * 14)()
    assert L.dw_layout(7, lay) == -1 and L.dw_layout(65, lay) == -1      # (k_power_extrap reads knots NK - 7 ..)
    for NK in (8, 11, 64):
        assert L.dw_layout(NK, lay) == 0
        v = list(lay)
        # make_layout(NM, NK): six knot tables of NK, then six coefficient tables of 4 (NK - 1),
        # the levels (6 NK), HaloFit's ln sigma^2 (NK), misc (8); the stride a multiple of 8
        assert [b - a for a, b in zip(v[0:5], v[1:6])] == [NK] * 5 and v[6] == v[5] + NK
        assert [b - a for a, b in zip(v[6:11], v[7:12])] == [4 * (NK - 1)] * 5
        assert v[12] == v[11] + 4 * (NK - 1) + 7 * NK
        assert v[13] % 8 == 0 and 0 <= v[13] - (v[12] + 8) < 8


@pytest.mark.skipif(not devcheck_build.have_hipcc(), reason="hipcc is not installed")
def test_devcell_compiles_and_exports():
    H = devcheck_build.HARNESSES["devcell"]
    others = [devcheck_build.HARNESSES[n] for n in ("devcheck", "devphys", "devproj", "devpower")]
    for o in others:
        devcheck_build.build(harness=o.name)
    stamps = [os.stat(o.so).st_mtime_ns for o in others]
    path = devcheck_build.build(harness="devcell")
    assert path == H.so and all(path != o.so for o in others)
    stamp = os.stat(path).st_mtime_ns
    assert devcheck_build.build(harness="devcell") == path
    assert os.stat(path).st_mtime_ns == stamp                 # (second call: nothing to do)
    assert [os.stat(o.so).st_mtime_ns for o in others] == stamps   # (the others: left alone)
    with open(H.hash) as f:
        assert f.read().strip() == devcheck_build.source_hash("devcell")
    L = ctypes.CDLL(path)
    for name in devcheck_build.CELL_ENTRY_POINTS:
        assert hasattr(L, name), name
    assert set(devcheck_build.VOID["devcell"]) <= set(devcheck_build.CELL_ENTRY_POINTS)
    assert devcheck_build.ALL_ENTRY_POINTS["devcell"] is devcheck_build.CELL_ENTRY_POINTS
    assert all(n.startswith("dl_") for n in devcheck_build.CELL_ENTRY_POINTS)
    # every entry point the tests name is declared (and so exported, above)
    here = os.path.dirname(os.path.abspath(__file__))
    for test in ("test_gpu_devcell.py", "test_devcell_cpu.py"):
        with open(os.path.join(here, test)) as f:
            named = set(re.findall(r"\b(dl_[a-z0-9_]+)\b", f.read()))
        assert named and named <= set(devcheck_build.CELL_ENTRY_POINTS), (test, named)
    # the package never loads it
    from chomp_amd import _lib
    assert not any("devcell" in src for src, _ in _lib.UNITS)
    # its hash covers the header chain and the plumbing it shares with devpower.hip
    for name in ("devcell", "devpower"):
        base = [os.path.basename(p) for p in devcheck_build.HARNESSES[name].headers]
        assert "power_setup.h" in base and "epoch_fill.h" in base, name
    base = [os.path.basename(p) for p in H.headers]
    for need in ("chomp_cov_kernels.h", "chomp_proj_kernels.h", "chomp_power_kernels.h",
                 "chomp_halo_kernels.h", "chomp_mass_kernels.h", "chomp_romberg.h",
                 "chomp_math.h", "special_tables.h", "chomp_mi355x.h"):
        assert need in base, need
    # the getters run on the host: the constants of the headers
    with open(os.path.join(_lib.CSRC, "chomp_proj_kernels.h")) as f:
        text = f.read()
    k = (ctypes.c_int * 5)()
    L.dl_constants(k)
    for i, name in enumerate(("kCellTabLevel", "kCellSplitLevel", "kCell4Level", "kCellDeepThreads")):
        assert k[i] == int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)), name
    assert k[4] == 160 * 1024 - 4096
    with open(os.path.join(_lib.CSRC, "chomp_romberg.h")) as f:
        assert L.dl_romberg_dump() == int(re.search(r"constexpr int kRombergDump = (\d+);", f.read()).group(1))
    assert L.dl_ptab_n() == 8192 and L.dl_pd_inputs() == 8


def test_harness_hash_covers_every_product_header(tmp_path, monkeypatch):
    """Each harness's hash covers the product headers it includes, transitively: devphys.hip
    and devproj.hip reach chomp_math.h through chomp_cov_kernels.h, and a change in any header of
    that chain changes their hashes; a header only they include leaves the first one's alone."""
    from chomp_amd import _lib
    for name in ("devphys", "devproj"):
        base = [os.path.basename(p) for p in devcheck_build.HARNESSES[name].headers]
        for need in ("chomp_cov_kernels.h", "chomp_proj_kernels.h", "chomp_power_kernels.h",
                     "chomp_halo_kernels.h", "chomp_mass_kernels.h", "chomp_romberg.h",
                     "chomp_math.h", "special_tables.h", "chomp_mi355x.h"):
            assert need in base, (name, need)
    first = [os.path.basename(p) for p in devcheck_build.HARNESSES["devcheck"].headers]
    assert sorted(first) == ["chomp_math.h", "chomp_romberg.h", "special_tables.h"]
    # a changed header (a scratch copy of the tree's csrc: no committed file is touched)
    import shutil
    root = tmp_path / "tree"
    shutil.copytree(os.path.join(_lib.CSRC), root / "chomp_amd" / "csrc")
    shutil.copytree(os.path.join(os.path.dirname(_lib.CSRC), "..", "include"), root / "include")
    os.makedirs(root / "tests" / "devcheck")
    for H in devcheck_build.HARNESSES.values():
        shutil.copy(H.src, root / "tests" / "devcheck")
    for shared in ("epoch_fill.h", "power_setup.h"):
        shutil.copy(os.path.join(devcheck_build.DIR, shared), root / "tests" / "devcheck")
    copies = {n: devcheck_build.Harness(n) for n in devcheck_build.HARNESSES}
    for H in copies.values():
        H.src = str(root / "tests" / "devcheck" / (H.name + ".hip"))
    monkeypatch.setattr(devcheck_build, "HARNESSES", copies)
    before = {n: devcheck_build.source_hash(n) for n in copies}
    with open(root / "chomp_amd" / "csrc" / "chomp_cov_kernels.h", "a") as f:
        f.write("// changed\n")
    after = {n: devcheck_build.source_hash(n) for n in copies}
    assert after["devphys"] != before["devphys"] and after["devcheck"] == before["devcheck"]
    assert after["devproj"] != before["devproj"]
    with open(root / "chomp_amd" / "csrc" / "chomp_math.h", "a") as f:
        f.write("// changed\n")
    last = {n: devcheck_build.source_hash(n) for n in copies}
    assert last["devphys"] != after["devphys"] and last["devcheck"] != after["devcheck"]
    assert last["devproj"] != after["devproj"]
    assert after["devpower"] != before["devpower"] and last["devpower"] != after["devpower"]
    # a harness's own source changes its hash alone
    with open(copies["devproj"].src, "a") as f:
        f.write("// changed\n")
    own = {n: devcheck_build.source_hash(n) for n in copies}
    assert own["devproj"] != last["devproj"]
    assert own["devphys"] == last["devphys"] and own["devcheck"] == last["devcheck"]
    assert own["devpower"] == last["devpower"]
    # the shared epoch filler changes the harnesses that include it, and only them
    with open(root / "tests" / "devcheck" / "epoch_fill.h", "a") as f:
        f.write("// changed\n")
    fill = {n: devcheck_build.source_hash(n) for n in copies}
    assert fill["devpower"] != own["devpower"] and fill["devphys"] != own["devphys"]
    assert fill["devcell"] != own["devcell"]
    assert fill["devproj"] == own["devproj"] and fill["devcheck"] == own["devcheck"]
    # ... and the plumbing devpower.hip and devcell.hip share those two
    with open(root / "tests" / "devcheck" / "power_setup.h", "a") as f:
        f.write("// changed\n")
    plumb = {n: devcheck_build.source_hash(n) for n in copies}
    assert plumb["devpower"] != fill["devpower"] and plumb["devcell"] != fill["devcell"]
    assert all(plumb[n] == fill[n] for n in ("devphys", "devproj", "devcheck"))
