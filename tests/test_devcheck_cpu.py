"""The device harnesses (tests/devcheck: devcheck.hip, the fp64 primitives and the wavefront
Romberg; devphys.hip, the halo-model physics; devproj.hip, the moment route of w(theta), the
bicubic tables and the quintic derivatives) compile for
gfx950 against the current headers and export every entry point the GPU tests
(test_gpu_devmath.py, test_gpu_romberg.py; test_gpu_devphys.py; test_gpu_devproj.py) use.  No GPU is needed: hipcc cross-compiles.  This
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
    # a harness's own source changes its hash alone
    with open(copies["devproj"].src, "a") as f:
        f.write("// changed\n")
    own = {n: devcheck_build.source_hash(n) for n in copies}
    assert own["devproj"] != last["devproj"]
    assert own["devphys"] == last["devphys"] and own["devcheck"] == last["devcheck"]
