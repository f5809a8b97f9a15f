"""CPU: the entries of the L1 FGINN matcher (vector_dist = L1: the f32 entries with a distance argument, the byte-row entries for the
SIFT family) exist in the library with the argument lists of include/modsx.h, and the host-only pieces -- the geometry rule of the
byte-row search, the argument checks that come before any device work -- behave as the header says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

F32 = ["modsx_ctx*", "constfloat*", "int", "constfloat*", "int", "int", "constdouble*", "double", "double", "int"]
DEBUG_TAIL = ["int", "int", "unsignedlonglong*", "unsignedchar*", "int*", "int*", "modsx_tentative**"]
# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_match_fginn_f32_dist": F32 + ["int", "modsx_tentative**"],
    "modsx_match_fginn_f32_dist_device": ["modsx_ctx*", "constvoid*", "int", "constvoid*", "int", "int", "constdouble*", "double", "double",
                                          "int", "int", "modsx_tentative**"],
    "modsx_match_regions_f32_dist": ["modsx_ctx*", "constmodsx_region*", "constfloat*", "int", "constmodsx_region*", "constfloat*", "int",
                                     "int", "constmodsx_pair_params*", "int", "modsx_pair_result*"],
    "modsx_debug_match_fginn_f32_dist": F32 + ["int"] + DEBUG_TAIL,
    "modsx_match_fginn_l1": ["modsx_ctx*", "constfloat*", "int", "constfloat*", "int", "constdouble*", "double", "double", "int",
                             "modsx_tentative**"],
    "modsx_match_fginn_l1_device": ["modsx_ctx*", "constvoid*", "int", "constvoid*", "int", "constdouble*", "double", "double", "int",
                                    "modsx_tentative**"],
    "modsx_match_regions_l1": ["modsx_ctx*", "constmodsx_region*", "constfloat*", "int", "constmodsx_region*", "constfloat*", "int",
                               "constmodsx_pair_params*", "modsx_pair_result*"],
    "modsx_debug_match_fginn_l1": ["modsx_ctx*", "constfloat*", "int", "constfloat*", "int", "constdouble*", "double", "double", "int"]
    + DEBUG_TAIL,
    "modsx_debug_fginn_l1_geometry": ["int", "int", "int", "int*"],
}
# the entries a `_dist` entry mirrors: its argument list is theirs plus one int
MIRRORS = {"modsx_match_fginn_f32_dist": ("modsx_match_fginn_f32", 10), "modsx_match_fginn_f32_dist_device": ("modsx_match_fginn_f32_device", 10),
           "modsx_match_regions_f32_dist": ("modsx_match_regions_f32", 9), "modsx_debug_match_fginn_f32_dist": ("modsx_debug_match_fginn_f32", 10)}


def _ctype_name(t):
    return {C.c_void_p: "ptr", C.c_int: "int", C.c_double: "double"}[t]


def _params(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    params = []
    for p in m.group(1).split(","):
        p = re.sub(r"\s+", " ", p.strip())
        p = re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", p)          # the parameter's name
        params.append(p.replace(" ", ""))
    return params


def test_symbols_exist_with_the_headers_argument_lists(modsx):
    hdr = open(os.path.join(ROOT, "include", "modsx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = modsx.lib()
    for name, want in DECLARED.items():
        params = _params(hdr, name)
        assert params == want, (name, params)
        assert name in modsx.EXPORTS and hasattr(L, name), name
        bound = [_ctype_name(t) for t in getattr(L, name).argtypes]
        assert bound == ["ptr" if w.endswith("*") else w for w in want], (name, bound)
    for name, (old, at) in MIRRORS.items():
        a = _params(hdr, old)
        assert _params(hdr, name) == a[:at] + ["int"] + a[at:], name
    assert re.search(r"enum\s*\{\s*MODSX_DIST_L2\s*=\s*0\s*,\s*MODSX_DIST_L1\s*=\s*1\s*\}\s*;", hdr)
    assert (modsx.DIST_L2, modsx.DIST_L1) == (0, 1)
    for method in ("match_fginn_l1", "match_fginn_l1_device", "debug_match_fginn_l1", "match_regions_l1"):
        assert callable(getattr(modsx.Context, method))
    import inspect
    for method in ("match_fginn_f32", "match_fginn_f32_device", "debug_match_fginn_f32", "match_regions_f32"):
        assert inspect.signature(getattr(modsx.Context, method)).parameters["dist"].default == modsx.DIST_L2
    assert callable(modsx.fginn_l1_geometry)


def test_l1_geometry_rules(modsx):
    rs = np.random.RandomState(5)
    sizes = [(1, 1), (1, 2), (257, 3), (4096, 20011), (2000000, 2000000), (100000, 7), (2049, 29185)]
    sizes += [(int(rs.randint(1, 9000)), int(rs.randint(1, 60000))) for _ in range(40)]
    for n1, n2 in sizes:
        for splits in (0, 1, 2, 3, 7, 64, 1 << 20):
            g = modsx.fginn_l1_geometry(n1, n2, splits)
            T, S, tps, tiles = g["tile"], g["splits"], g["tiles_per_split"], g["tiles"]
            assert T == 128 and g["DK"] == 32                               # 128 rows of 32 dwords: 16 KiB of LDS
            assert tiles * T >= n2 > (tiles - 1) * T                        # tiles cover n2, none is empty
            assert 1 <= S <= tiles and S * tps >= tiles > (S - 1) * tps     # no empty split
            assert g["workgroups"] == S * ((n1 + 255) // 256)
            if splits > 0:
                assert S <= splits
            if splits == 1:
                assert S == 1
            if splits >= tiles:
                assert S == tiles and tps == 1
            assert g == modsx.fginn_l1_geometry(n1, n2, splits)             # one function of its arguments
            # the split rule is the f32 search's at the same tile count
            f = modsx.fginn32_geometry(n1, n2, 32, splits)
            assert (f["tile"], f["splits"], f["tiles_per_split"]) == (T, S, tps)
    assert modsx.fginn_l1_geometry(4096, 20011) == modsx.fginn_l1_geometry(4096, 20011, 0)
    g = modsx.fginn_l1_geometry(2049, 29185)
    assert g["splits"] >= 2 and g["tiles_per_split"] == 2 and modsx.fginn_l1_geometry(2049, 29184)["tiles_per_split"] == 1


def test_geometry_refusals(modsx):
    for n1, n2 in ((0, 5), (5, 0), (-1, 5), (5, 2000001), (2000001, 5)):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+"):
            modsx.fginn_l1_geometry(n1, n2)
    with pytest.raises(RuntimeError, match=r"\(-1\): .+"):
        modsx.fginn_l1_geometry(5, 5, -1)


def test_refusals_that_need_no_device(modsx):
    """argument checks of the device entries come before any device work: a null context handle would crash otherwise"""
    L = modsx.lib()
    out = C.c_void_p()
    pos = np.zeros((8, 2))
    ptr = C.c_void_p(4096)                      # never dereferenced
    P = pos.ctypes.data_as(C.c_void_p)

    def refused(rc, what):
        assert rc == -1, what
        assert what in L.modsx_last_error().decode(), (what, L.modsx_last_error())

    ctx = C.c_void_p(1)                         # not a context: the checks below must not touch it
    for dist in (2, -1, 7):
        refused(L.modsx_match_fginn_f32_dist_device(ctx, ptr, 4, ptr, 8, 36, P, 0.8, 30.0, 50, dist, C.byref(out)), "dist")
    for dim in (6, 0, 260):
        refused(L.modsx_match_fginn_f32_dist_device(ctx, ptr, 4, ptr, 8, dim, P, 0.8, 30.0, 50, 1, C.byref(out)), "dim")
    for ratio in (1.0, 1.5, -1.0, float("inf")):
        refused(L.modsx_match_fginn_f32_dist_device(ctx, ptr, 4, ptr, 8, 36, P, ratio, 30.0, 50, 1, C.byref(out)), "all points")
        refused(L.modsx_match_fginn_l1_device(ctx, ptr, 4, ptr, 8, P, ratio, 30.0, 50, C.byref(out)), "all points")
    refused(L.modsx_match_fginn_l1_device(ctx, ptr, 4, ptr, 8, P, float("nan"), 30.0, 50, C.byref(out)), "NaN")
    for nn in (1, 257, 0, -3):
        refused(L.modsx_match_fginn_l1_device(ctx, ptr, 4, ptr, 8, P, 0.8, 30.0, nn, C.byref(out)), "nn")
        refused(L.modsx_match_fginn_f32_dist_device(ctx, ptr, 4, ptr, 8, 36, P, 0.8, 30.0, nn, 1, C.byref(out)), "nn")
    refused(L.modsx_match_fginn_l1_device(ctx, ptr, 2000001, ptr, 8, P, 0.8, 30.0, 50, C.byref(out)), "2 000 000")
    refused(L.modsx_match_fginn_l1_device(ctx, ptr, 4, ptr, -1, P, 0.8, 30.0, 50, C.byref(out)), "negative")
    refused(L.modsx_match_fginn_l1_device(ctx, None, 4, ptr, 8, P, 0.8, 30.0, 50, C.byref(out)), "null")
    refused(L.modsx_match_fginn_f32_dist_device(ctx, C.c_void_p(4098), 4, ptr, 8, 36, P, 0.8, 30.0, 50, 1, C.byref(out)), "aligned")
