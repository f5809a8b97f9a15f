"""CPU: the entries of the f32 FGINN matcher (MatchFlannFGINN on float rows of any width) exist in the library with the argument
lists of include/modsx.h, and its host-only pieces -- the geometry rule and the argument checks -- behave as the header says."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_match_fginn_f32": ["modsx_ctx*", "constfloat*", "int", "constfloat*", "int", "int", "constdouble*", "double", "double", "int",
                              "modsx_tentative**"],
    "modsx_match_fginn_f32_device": ["modsx_ctx*", "constvoid*", "int", "constvoid*", "int", "int", "constdouble*", "double", "double",
                                     "int", "modsx_tentative**"],
    "modsx_match_regions_f32": ["modsx_ctx*", "constmodsx_region*", "constfloat*", "int", "constmodsx_region*", "constfloat*", "int", "int",
                                "constmodsx_pair_params*", "modsx_pair_result*"],
    "modsx_debug_match_fginn_f32": ["modsx_ctx*", "constfloat*", "int", "constfloat*", "int", "int", "constdouble*", "double", "double",
                                    "int", "int", "int", "unsignedlonglong*", "unsignedchar*", "int*", "int*", "modsx_tentative**"],
    "modsx_debug_fginn32_geometry": ["int", "int", "int", "int", "int*"],
    "modsx_debug_fginn32_dpass": ["constfloat*", "constdouble*", "int", "float*"],
}


def _ctype_name(t):
    import ctypes as C
    return {C.c_void_p: "ptr", C.c_int: "int", C.c_double: "double"}[t]


def test_symbols_exist_with_the_headers_argument_lists(modsx):
    hdr = open(os.path.join(ROOT, "include", "modsx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
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
    assert re.search(r"#define\s+MODSX_FGINN32_MAX_DIM\s+256\b", hdr)
    for method in ("match_fginn_f32", "match_fginn_f32_device", "match_regions_f32", "debug_match_fginn_f32"):
        assert callable(getattr(modsx.Context, method))
    assert callable(modsx.fginn32_geometry)


@pytest.mark.parametrize("dim", [4, 8, 32, 36, 64, 68, 128, 132, 144, 192, 196, 200, 256])
def test_geometry_rules(modsx, dim):
    rs = np.random.RandomState(dim)
    sizes = [(1, 1), (1, 2), (257, 3), (4096, 20011), (2000000, 2000000), (100000, 7)]
    sizes += [(int(rs.randint(1, 9000)), int(rs.randint(1, 60000))) for _ in range(20)]
    for n1, n2 in sizes:
        for splits in (0, 1, 2, 3, 7, 64, 1 << 20):
            g = modsx.fginn32_geometry(n1, n2, dim, splits)
            T, S, tps, tiles = g["tile"], g["splits"], g["tiles_per_split"], g["tiles"]
            assert g["DK"] >= dim and g["DK"] in (32, 64, 128, 192, 256) and (g["DK"] == 32 or g["DK"] - dim < 64)   # the width class
            assert T >= 1 and T * g["DK"] % 1024 == 0                     # a tile is whole float4s for 256 threads
            assert tiles * T >= n2 > (tiles - 1) * T                      # tiles cover n2, none is empty
            assert 1 <= S <= tiles                                        # S <= tiles
            assert S * tps >= tiles > (S - 1) * tps                       # no empty split
            assert g["workgroups"] == S * ((n1 + 255) // 256)
            if splits > 0:
                assert S <= splits
            if splits == 1:
                assert S == 1
            if splits >= tiles:
                assert S == tiles and tps == 1
    # one function of its arguments
    assert modsx.fginn32_geometry(4096, 20011, dim) == modsx.fginn32_geometry(4096, 20011, dim, 0)


def test_geometry_refusals(modsx):
    for dim in (0, 6, 260, -4, 2, 258):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+dim"):
            modsx.fginn32_geometry(10, 10, dim)
    for n1, n2 in ((0, 5), (5, 0), (-1, 5), (5, 2000001), (2000001, 5)):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+"):
            modsx.fginn32_geometry(n1, n2, 128)
    with pytest.raises(RuntimeError, match=r"\(-1\): .+"):
        modsx.fginn32_geometry(5, 5, 128, -1)
    assert modsx.fginn32_geometry(2000000, 2000000, 256)["DK"] == 256


def test_dpass_refusals(modsx):
    for d0, ratio in ((-1.0, 0.5), (float("inf"), 0.5), (float("nan"), 0.5), (1.0, float("nan"))):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+"):
            modsx.fginn32_dpass([d0], [ratio])
    assert modsx.fginn32_dpass([1.0], [0.8])[0] == np.float32(1.5625)       # 1 / 0.64
