"""CPU: the entries of the SURF descriptor exist in the library with the argument lists of include/modsx.h, and what needs no
device -- the tables and the refusals that come before any context is touched -- behaves as the header says."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

REGIONS = ["modsx_ctx*", "constmodsx_image*", "constmodsx_region*", "int", "double", "int", "int", "int"]
# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_surf_patches": ["modsx_ctx*", "constfloat*", "int", "int", "double", "float*"],
    "modsx_surf_patches_device": ["modsx_ctx*", "constvoid*", "int", "int", "double", "void*"],
    "modsx_describe_regions_surf": REGIONS + ["float*"],
    "modsx_describe_regions_surf_device": REGIONS + ["void*"],
    "modsx_surf_tables": ["int", "double", "int*", "int*", "float*", "float*", "int*"],
    "modsx_surf_counters": ["modsx_ctx*", "long*", "int"],
}


def _ctype_name(t):
    return {C.c_void_p: "ptr", C.c_int: "int", C.c_double: "double"}[t]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modsx.h")).read(), flags=re.S)


def _params(name, hdr):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_symbols_exist_with_the_headers_argument_lists(modsx):
    hdr = _header()
    L = modsx.lib()
    for name, want in DECLARED.items():
        params = [re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", p).replace(" ", "") for p in _params(name, hdr)]
        assert params == want, (name, params)
        assert name in modsx.EXPORTS and hasattr(L, name), name
        bound = [_ctype_name(t) for t in getattr(L, name).argtypes]
        assert bound == ["ptr" if w.endswith("*") else w for w in want], (name, bound)
    assert re.search(r"#define\s+MODSX_SURF_DIM\s+64\b", hdr) and modsx.SURF_DIM == 64
    for method in ("surf_patches", "surf_patches_device", "describe_regions_surf", "describe_regions_surf_device", "surf_counters"):
        assert callable(getattr(modsx.Context, method))
    assert callable(modsx.surf_tables) and modsx.SURF_COUNTERS == ("calls", "patches", "sub_batches")


def test_same_arguments_as_describe_regions_liop():
    """the region entries mirror the LIOP block, the patch entries add mrSize behind patchSize"""
    hdr = _header()
    names = lambda fn: [re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", p).group(1) for p in _params(fn, hdr)]      # noqa: E731
    assert names("modsx_describe_regions_surf") == names("modsx_describe_regions_liop")
    assert names("modsx_describe_regions_surf_device") == names("modsx_describe_regions_liop_device")
    assert names("modsx_surf_patches") == ["ctx", "patches", "n", "patchSize", "mrSize", "desc"]
    assert names("modsx_surf_patches_device") == ["ctx", "dev_patches", "n", "patchSize", "mrSize", "dev_desc"]


def test_tables(modsx):
    L = modsx.lib()
    t = modsx.surf_tables(20.5)
    # scale 2: samples every 2 px around 21, xs = 21 + 2 ix, the weights fall off with the distance to the sub-region's centre
    assert list(t["sample_x"]) == list(range(-3, 45, 2)) == list(t["sample_y"]) and t["haar_size"] == 4
    assert t["w1"].shape == (16, 81) and t["w2"].shape == (16,) and (t["w1"] > 0).all() and (t["w2"] > 0).all()
    for q in range(16):
        w = t["w1"][q].reshape(9, 9)
        assert np.array_equal(w, w.T) and w.argmax() == 5 * 9 + 5                  # k = i + 5, l = j + 5: the centre sample
    w2 = t["w2"].reshape(4, 4)
    assert np.array_equal(w2, w2.T) and np.array_equal(w2, w2[::-1, ::-1]) and w2[1, 1] == w2.max()
    # any pointer may be left out
    hs = np.zeros(1, np.int32)
    assert L.modsx_surf_tables(41, C.c_double(5.1962), None, None, None, None, hs.ctypes.data_as(C.c_void_p)) == 0 and hs[0] == 16
    assert L.modsx_surf_tables(41, C.c_double(5.1962), None, None, None, None, None) == 0
    assert modsx.surf_tables(100.0)["haar_size"] == 0


def test_refusals_without_a_device(modsx):
    L = modsx.lib()
    for ps in (0, 40, 42, -41):
        assert L.modsx_surf_tables(ps, C.c_double(5.1962), None, None, None, None, None) == -1 and b"41" in L.modsx_last_error()
    for mr in (0.0, -5.1962, float("nan"), float("inf"), -float("inf"), 41.0 / 1025.0, 1e-300):
        assert L.modsx_surf_tables(41, C.c_double(mr), None, None, None, None, None) == -1, mr
        assert b"mrSize" in L.modsx_last_error()
    assert L.modsx_surf_tables(41, C.c_double(41.0 / 1024.0), None, None, None, None, None) == 0         # the bound itself
    buf = np.zeros(1681, np.float32).ctypes.data_as(C.c_void_p)
    # a null context is refused before anything else is looked at
    assert L.modsx_surf_patches(None, buf, 1, 41, C.c_double(5.1962), buf) == -1
    assert L.modsx_surf_patches_device(None, buf, 1, 41, C.c_double(5.1962), buf) == -1
    assert L.modsx_describe_regions_surf(None, buf, buf, 1, C.c_double(5.1962), 41, 0, 1, buf) == -1
    assert L.modsx_describe_regions_surf_device(None, buf, buf, 1, C.c_double(5.1962), 41, 0, 1, buf) == -1
    assert L.modsx_surf_counters(None, buf, 3) == -1
    assert b"null argument" in L.modsx_last_error()
