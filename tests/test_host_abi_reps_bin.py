"""CPU: the ABI of the binary classes of stored representations (include/modsx.h: modsx_rep_append_bin and what follows it)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> the parameter types of the declaration, spaces removed
NEW = {
    "modsx_rep_append_bin": ["modsx_ctx*", "modsx_rep*", "int", "int", "constmodsx_region*", "constvoid*", "int", "int", "int"],
    "modsx_rep_append_bin_device": ["modsx_ctx*", "modsx_rep*", "int", "int", "constmodsx_region*", "constvoid*", "int", "int"],
    "modsx_rep_class_bin": ["modsx_ctx*", "constmodsx_rep*", "int", "int", "modsx_region**", "unsignedchar**", "int*"],
    "modsx_rep_match_hamming": ["modsx_ctx*", "constmodsx_rep*", "constmodsx_rep*", "int", "int", "double", "modsx_tentative**"],
    "modsx_rep_match_group_hamming": ["modsx_ctx*", "constmodsx_rep*", "constmodsx_rep*const*", "int", "int", "int", "double",
                                      "modsx_tentative**", "int*"],
    "modsx_debug_hamming_group_geometry": ["int", "constint*", "int", "int", "int*", "int*", "int*", "int"],
    "modsx_hamming_group_counters": ["modsx_ctx*", "long*", "int"],
    "modsx_rep_class_order": ["int", "int"],
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


def test_binary_class_symbols_are_declared_listed_and_exported_with_these_arguments(modsx):
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
    for name in ("append_bin", "append_bin_device", "regions_bin"):
        assert hasattr(modsx.Rep, name), name
    for name in ("rep_match_hamming", "rep_match_group_hamming", "hamming_group_counters"):
        assert hasattr(modsx.Context, name), name
    for name in ("hamming_group_geometry", "rep_class_order", "match_reps"):
        assert hasattr(modsx, name), name


def test_enum_values_and_unchanged_layouts(modsx):
    hdr = _header()
    want = dict(MODSX_DET_ORB=4, MODSX_DESC_BRISK=16, MODSX_DESC_FREAK=17, MODSX_DESC_ORB=18,
                MODSX_DESC_CAFFE=8, MODSX_DESC_SURF=12, MODSX_DESC_SIFT=0, MODSX_DESC_HALF_ROOT_SIFT=3, MODSX_DET_MSER=3)
    for name, v in want.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), hdr), name
    assert re.search(r"#define\s+MODSX_DET_SURF\s+6\b", hdr)
    assert re.search(r"#define\s+MODSX_MAX_DESC\s+4\b", hdr)
    assert re.search(r"#define\s+MODSX_HAMMING_MAX_BYTES\s+64\b", hdr)
    assert re.search(r"#define\s+MODSX_REP_BIN_FIRST_ROWS\s+%d\b" % modsx.REP_BIN_FIRST_ROWS, hdr) and modsx.REP_BIN_FIRST_ROWS == 4096
    assert (modsx.DET_ORB, modsx.DESC_BRISK, modsx.DESC_FREAK, modsx.DESC_ORB) == (4, 16, 17, 18)
    assert (modsx.DET_HESSIAN, modsx.DET_MSER, modsx.DET_SURF) == (0, 3, 6)
    assert len(modsx.HAMMING_GROUP_COUNTERS) == 4
    # no public struct changes
    assert re.search(r"typedef\s+struct\s*\{\s*int\s+detector\s*,\s*desc_type\s*;\s*double\s+ratio\s*;\s*\}\s*modsx_rep_class_sel\s*;", hdr)
    assert C.sizeof(modsx.RepClassSel) == 16
    assert C.sizeof(modsx.PairParams) == 328 and C.sizeof(modsx.PairResult) == 128 and C.sizeof(modsx.LadderStep) == 80
