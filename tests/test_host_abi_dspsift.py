"""CPU: the entries of the raw SIFT histograms, the f32 SIFT norm and DSP-SIFT exist in the library with the argument lists of
include/modsx.h, and the refusals that come before any context is touched behave as the header says."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

REGIONS = ["modsx_ctx*", "constmodsx_image*", "constmodsx_region*", "int", "double", "int", "int", "int"]
DSP = ["int", "double", "double", "double"]
# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_describe_regions_raw": REGIONS + ["float*"],
    "modsx_describe_regions_raw_device": REGIONS + ["void*"],
    "modsx_sift_norm_rows": ["modsx_ctx*", "constfloat*", "int", "double", "float*"],
    "modsx_sift_norm_rows_device": ["modsx_ctx*", "constvoid*", "int", "double", "void*"],
    "modsx_describe_regions_dspsift": REGIONS + DSP + ["float*"],
    "modsx_describe_regions_dspsift_device": REGIONS + DSP + ["void*"],
    "modsx_dsp_counters": ["modsx_ctx*", "long*", "int"],
}


def _ctype_name(t):
    return {C.c_void_p: "ptr", C.c_int: "int", C.c_double: "double"}[t]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modsx.h")).read(), flags=re.S)


def _names(fn):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % fn, _header())
    assert m, fn
    return [re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", p.strip()).group(1) for p in m.group(1).split(",")]


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
    for method in ("describe_regions_raw", "sift_norm_rows", "sift_norm_rows_device", "describe_regions_dspsift", "dsp_counters"):
        assert callable(getattr(modsx.Context, method))
    assert modsx.DSP_COUNTERS == ("calls", "regions", "scale_passes")


def test_argument_names(modsx):
    """the raw entry takes the arguments of modsx_describe_regions minus desc_type / maxBinValue; the DSP-SIFT entry those, then
    the pooling parameters and the norm's clip"""
    base = _names("modsx_describe_regions")
    front = [n for n in base[:-1] if n not in ("desc_type", "maxBinValue")]
    assert _names("modsx_describe_regions_raw") == front + ["hist"]
    assert _names("modsx_describe_regions_raw_device") == front + ["dev_hist"]
    assert _names("modsx_describe_regions_dspsift") == front + ["numScales", "startCoef", "endCoef", "maxBinValue", "desc"]
    assert _names("modsx_describe_regions_dspsift_device") == front + ["numScales", "startCoef", "endCoef", "maxBinValue", "dev_desc"]
    assert _names("modsx_sift_norm_rows") == ["ctx", "rows", "n", "maxBinValue", "out"]


def test_describe_regions_takes_no_new_type():
    hdr = open(os.path.join(ROOT, "include", "modsx.h")).read()
    assert not re.search(r"#define\s+MODSX_DESC_\w*DSP", hdr)


def test_refusals_without_a_device(modsx):
    L = modsx.lib()
    buf = np.zeros(256, np.float32).ctypes.data_as(C.c_void_p)
    one, d = C.c_double(1.0), C.c_double
    # a null context is refused before anything else is looked at
    assert L.modsx_describe_regions_raw(None, buf, buf, 1, one, 41, 0, 1, buf) == -1
    assert L.modsx_describe_regions_raw_device(None, buf, buf, 1, one, 41, 0, 1, buf) == -1
    assert L.modsx_sift_norm_rows(None, buf, 1, d(0.2), buf) == -1
    assert L.modsx_sift_norm_rows_device(None, buf, 1, d(0.2), buf) == -1
    assert L.modsx_describe_regions_dspsift(None, buf, buf, 1, one, 41, 0, 1, 3, d(0.5), d(1.5), d(0.2), buf) == -1
    assert L.modsx_describe_regions_dspsift_device(None, buf, buf, 1, one, 41, 0, 1, 3, d(0.5), d(1.5), d(0.2), buf) == -1
    assert L.modsx_dsp_counters(None, buf, 3) == -1
    assert b"null argument" in L.modsx_last_error()
