"""CPU: the ABI of the float classes of stored representations (include/modsx.h: modsx_rep_append_f32 and what follows it)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> the parameter types of the declaration, spaces removed
NEW = {
    "modsx_rep_append_f32": ["modsx_ctx*", "modsx_rep*", "int", "int", "constmodsx_region*", "constfloat*", "int", "int"],
    "modsx_rep_describe_append": ["modsx_ctx*", "modsx_rep*", "int", "int", "constmodsx_image*", "constmodsx_region*", "int", "double",
                                  "int", "int", "int", "constint*"],
    "modsx_rep_class_f32": ["modsx_ctx*", "constmodsx_rep*", "int", "int", "modsx_region**", "float**", "int*"],
    "modsx_rep_match_fginn_f32": ["modsx_ctx*", "constmodsx_rep*", "constmodsx_rep*", "int", "int", "double", "double", "int",
                                  "modsx_tentative**"],
    "modsx_rep_match_group_f32": ["modsx_ctx*", "constmodsx_rep*", "constmodsx_rep*const*", "int", "int", "int", "double", "double", "int",
                                  "modsx_tentative**", "int*"],
    "modsx_rep_class_rank": ["int", "int"],
    "modsx_debug_fginn32_group_geometry": ["int", "constint*", "int", "int", "int*", "int*", "int*", "int"],
    "modsx_fginn32_group_counters": ["modsx_ctx*", "long*", "int"],
}
CTYPE = {"int": C.c_int, "double": C.c_double}


def _header():
    hdr = open(os.path.join(ROOT, "include", "modsx.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _params(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = re.sub(r"\s+", " ", p.strip())
        p = re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", p)          # the parameter's name
        out.append(p.replace(" ", ""))
    return out


def test_float_class_symbols_are_declared_listed_and_exported_with_these_arguments(modsx):
    hdr = _header()
    L = modsx.lib()
    for name, want in NEW.items():
        assert _params(hdr, name) == want, (name, _params(hdr, name))
        assert name in modsx.EXPORTS, name
        fn = getattr(L, name)
        # the wrapper's argument list has the header's length; scalars have the header's type, everything else is a pointer
        assert len(fn.argtypes) == len(want), name
        for a, w in zip(fn.argtypes, want):
            assert a is CTYPE.get(w, C.c_void_p), (name, w, a)
    for name in ("append_f32", "describe_append", "class_f32", "count_f32"):
        assert hasattr(modsx.Rep, name), name
    for name in ("rep_match_fginn_f32", "rep_match_group_f32", "fginn32_group_counters"):
        assert hasattr(modsx.Context, name), name
    for name in ("rep_class_rank", "fginn32_group_geometry"):
        assert hasattr(modsx, name), name


def test_enum_values_and_unchanged_layouts(modsx):
    hdr = _header()
    want = dict(MODSX_DESC_CAFFE=8, MODSX_DESC_DAISY=9, MODSX_DESC_LIOP=10, MODSX_DESC_MROGH=11, MODSX_DESC_SURF=12,
                MODSX_DESC_SIFT=0, MODSX_DESC_ROOT_SIFT=1, MODSX_DESC_HALF_SIFT=2, MODSX_DESC_HALF_ROOT_SIFT=3)
    for name, v in want.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), hdr), name
    assert re.search(r"#define\s+MODSX_MAX_DESC\s+4\b", hdr)
    assert re.search(r"#define\s+MODSX_REP_F32_FIRST_ROWS\s+%d\b" % modsx.REP_F32_FIRST_ROWS, hdr)
    assert (modsx.DESC_CAFFE, modsx.DESC_DAISY, modsx.DESC_LIOP, modsx.DESC_MROGH, modsx.DESC_SURF) == (8, 9, 10, 11, 12)
    assert (modsx.DET_HESSIAN, modsx.DET_MSER, modsx.DET_SURF) == (0, 3, 6)
    assert re.search(r"typedef\s+struct\s*\{\s*int\s+detector\s*,\s*desc_type\s*;\s*double\s+ratio\s*;\s*\}\s*modsx_rep_class_sel\s*;", hdr)
    assert C.sizeof(modsx.RepClassSel) == 16
    assert C.sizeof(modsx.PairParams) == 328 and C.sizeof(modsx.PairResult) == 128 and C.sizeof(modsx.LadderStep) == 80
