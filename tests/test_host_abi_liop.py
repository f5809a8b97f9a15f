"""CPU: the entries of the patch-out front end and of the LIOP descriptor exist in the library with the argument lists of
include/modsx.h, and what needs no device -- the tables and the refusals that come before any context is touched -- behaves as
the header says."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

REGIONS = ["modsx_ctx*", "constmodsx_image*", "constmodsx_region*", "int", "double", "int", "int", "int"]
# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_extract_patches": REGIONS + ["float*"],
    "modsx_extract_patches_device": REGIONS + ["void*"],
    "modsx_liop_patches": ["modsx_ctx*", "constfloat*", "int", "int", "float*"],
    "modsx_liop_patches_device": ["modsx_ctx*", "constvoid*", "int", "int", "void*"],
    "modsx_describe_regions_liop": REGIONS + ["float*"],
    "modsx_describe_regions_liop_device": REGIONS + ["void*"],
    "modsx_liop_tables": ["int", "int*", "double*", "double*", "int"],
    "modsx_debug_liop": ["modsx_ctx*", "constfloat*", "int", "int", "float*", "int*", "int*"],
    "modsx_liop_counters": ["modsx_ctx*", "long*", "int"],
}


def _ctype_name(t):
    return {C.c_void_p: "ptr", C.c_int: "int", C.c_double: "double"}[t]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modsx.h")).read(), flags=re.S)


def test_symbols_exist_with_the_headers_argument_lists(modsx):
    hdr = _header()
    L = modsx.lib()
    for name, want in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        params = []
        for p in m.group(1).split(","):
            p = re.sub(r"\s+", " ", p.strip())
            p = re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", p)          # the parameter's name
            params.append(p.replace(" ", ""))
        assert params == want, (name, params)
        assert name in modsx.EXPORTS and hasattr(L, name), name
        bound = [_ctype_name(t) for t in getattr(L, name).argtypes]
        assert bound == ["ptr" if w.endswith("*") else w for w in want], (name, bound)
    assert re.search(r"#define\s+MODSX_LIOP_DIM\s+144\b", hdr) and modsx.LIOP_DIM == 144
    assert re.search(r"#define\s+MODSX_LIOP_PIXELS\s+673\b", hdr) and modsx.LIOP_PIXELS == 673
    for method in ("extract_patches", "liop_patches", "liop_patches_device", "describe_regions_liop", "debug_liop", "liop_counters"):
        assert callable(getattr(modsx.Context, method))
    assert callable(modsx.liop_tables) and len(modsx.LIOP_COUNTERS) == 4


def test_same_arguments_as_describe_regions(modsx):
    """modsx_extract_patches / modsx_describe_regions_liop: the arguments of modsx_describe_regions minus desc_type / maxBinValue"""
    L = modsx.lib()
    m = re.search(r"\bint\s+modsx_describe_regions\s*\(([^)]*)\)\s*;", _header())
    names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", p.strip()).group(1) for p in m.group(1).split(",")]
    assert names == ["ctx", "img", "regs", "n", "mrSize", "patchSize", "fast_extraction", "photoNorm", "desc_type", "maxBinValue", "desc"]
    for fn in ("modsx_extract_patches", "modsx_describe_regions_liop"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % fn, _header())
        got = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", p.strip()).group(1) for p in m.group(1).split(",")]
        assert got[:-1] == [n for n in names[:-1] if n not in ("desc_type", "maxBinValue")], fn
        assert len(getattr(L, fn).argtypes) == len(names) - 2


def test_tables(modsx):
    L = modsx.lib()
    pixels, sx, sy = modsx.liop_tables()
    assert len(pixels) == 673 and sx.shape == (673, 4) == sy.shape
    assert (np.diff(pixels) > 0).all() and pixels.min() > 0 and pixels.max() < 1681          # raster order
    y, x = pixels // 41 - 20, pixels % 41 - 20
    assert ((x * x + y * y) <= 213).all() and int(((np.mgrid[-20:21, -20:21] ** 2).sum(0) <= 213).sum()) == 673
    # radius 6 around the pixel, the first sample straight outwards
    assert np.allclose(np.hypot(sx - (x[:, None] + 20), sy - (y[:, None] + 20)), 6.0, atol=1e-12)
    # any of the three outputs may be left out; cap cuts the lists, the count is returned whole
    assert L.modsx_liop_tables(41, None, None, None, 0) == 673
    few = np.full(8, -1, np.int32)
    assert L.modsx_liop_tables(41, few.ctypes.data_as(C.c_void_p), None, None, 5) == 673
    assert list(few[:5]) == list(pixels[:5]) and list(few[5:]) == [-1] * 3


def test_refusals_without_a_device(modsx):
    L = modsx.lib()
    for ps in (0, 40, 42, -41):
        assert L.modsx_liop_tables(ps, None, None, None, 0) == -1 and b"41" in L.modsx_last_error()
    assert L.modsx_liop_tables(41, None, None, None, -1) == -1
    buf = np.zeros(1681, np.float32).ctypes.data_as(C.c_void_p)
    # a null context is refused before anything else is looked at
    assert L.modsx_extract_patches(None, buf, buf, 1, C.c_double(1.0), 41, 0, 1, buf) == -1
    assert L.modsx_extract_patches_device(None, buf, buf, 1, C.c_double(1.0), 41, 0, 1, buf) == -1
    assert L.modsx_describe_regions_liop(None, buf, buf, 1, C.c_double(1.0), 41, 0, 1, buf) == -1
    assert L.modsx_describe_regions_liop_device(None, buf, buf, 1, C.c_double(1.0), 41, 0, 1, buf) == -1
    assert L.modsx_liop_patches(None, buf, 1, 41, buf) == -1
    assert L.modsx_liop_patches_device(None, buf, 1, 41, buf) == -1
    assert L.modsx_debug_liop(None, buf, 1, 41, buf, buf, buf) == -1
    assert L.modsx_liop_counters(None, buf, 4) == -1
    assert b"null argument" in L.modsx_last_error()
