"""CPU: the entries of the learned-descriptor front end exist in the library with the argument lists of include/modsx.h, and
what needs no device -- the defaults, the job table, the launch geometry and the refusals that come before any context is
touched -- behaves as the header says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import caffe_cases as Cs
import caffe_model as M
from conftest import ROOT

PATCHES = ["modsx_ctx*", "constmodsx_image*const*", "int", "constmodsx_region*", "int", "constmodsx_caffe_params*"]
APPEND = ["modsx_ctx*", "modsx_rep*", "int", "int", "constmodsx_region*"]
# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_caffe_patches": PATCHES + ["float*", "unsignedchar*"],
    "modsx_caffe_patches_device": PATCHES + ["void*", "unsignedchar*"],
    "modsx_caffe_jobs": ["constmodsx_region*", "int", "constmodsx_caffe_params*", "int", "int", "float*"],
    "modsx_debug_caffe_geometry": ["int", "int", "int*"],
    "modsx_caffe_norm_rows": ["modsx_ctx*", "constfloat*", "int", "int", "int", "float*"],
    "modsx_caffe_norm_rows_device": ["modsx_ctx*", "constvoid*", "int", "int", "int", "void*"],
    "modsx_caffe_counters": ["modsx_ctx*", "long*", "int"],
    "modsx_rep_append_f32_device": APPEND + ["constvoid*", "int", "int"],
    "modsx_rep_append_f32": APPEND + ["constfloat*", "int", "int"],
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modsx.h")).read(), flags=re.S)


def _params(name, hdr):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_exist_with_the_headers_argument_lists(modsx):
    hdr = _header()
    L = modsx.lib()
    for name, want in DECLARED.items():
        params = [re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", p).replace(" ", "") for p in _params(name, hdr)]
        assert params == want, (name, params)
        assert name in modsx.EXPORTS and hasattr(L, name), name
        bound = [{C.c_void_p: "ptr", C.c_int: "int"}[t] for t in getattr(L, name).argtypes]
        assert bound == ["ptr" if w.endswith("*") else w for w in want], (name, bound)
    assert re.search(r"\bvoid\s+modsx_default_caffe_params\s*\(\s*modsx_caffe_params\s*\*\s*p\s*\)\s*;", hdr)
    assert "modsx_default_caffe_params" in modsx.EXPORTS and hasattr(L, "modsx_default_caffe_params")
    assert re.search(r"#define\s+MODSX_CAFFE_MAX_PATCH\s+255\b", hdr) and modsx.CAFFE_MAX_PATCH == 255
    assert re.search(r"#define\s+MODSX_CAFFE_MAX_DIM\s+4096\b", hdr) and modsx.CAFFE_MAX_DIM == 4096
    m = re.search(r"MODSX_CAFFE_NORM_L2\s*=\s*(\d+)\s*,\s*MODSX_CAFFE_NORM_L1\s*=\s*(\d+)\s*,\s*MODSX_CAFFE_NORM_ROOTL2\s*=\s*(\d+)\s*,"
                  r"\s*MODSX_CAFFE_NORM_NONE\s*=\s*(\d+)", hdr)
    assert tuple(int(x) for x in m.groups()) == (modsx.CAFFE_NORM_L2, modsx.CAFFE_NORM_L1, modsx.CAFFE_NORM_ROOTL2, modsx.CAFFE_NORM_NONE)
    assert (modsx.CAFFE_NORM_L2, modsx.CAFFE_NORM_L1, modsx.CAFFE_NORM_ROOTL2, modsx.CAFFE_NORM_NONE) == \
        (M.NORM_L2, M.NORM_L1, M.NORM_ROOTL2, M.NORM_NONE)
    assert modsx.CAFFE_NORMS == {"L2": 0, "L1": 1, "RootL2": 2, "none": 3}
    for method in ("caffe_patches", "caffe_norm_rows", "caffe_norm_rows_device", "caffe_counters"):
        assert callable(getattr(modsx.Context, method))
    assert callable(modsx.Rep.append_f32_device) and callable(modsx.caffe_jobs) and callable(modsx.caffe_geometry)
    assert modsx.CAFFE_COUNTERS == ("calls", "regions", "border_regions", "launches")
    from mods_amd import learned
    assert callable(learned.describe_learned)


def test_default_params(modsx):
    p = modsx.caffe_params()
    assert p.mrSize == 3.0 * 3.0 ** 0.5 and p.patchSize == 41 and list(p.mean) == [104.0, 117.0, 123.0]
    assert C.sizeof(modsx.CaffeParams) == 40
    m = re.search(r"typedef struct modsx_caffe_params \{(.*?)\} modsx_caffe_params;", _header(), flags=re.S)
    assert [re.sub(r"\s+", " ", f.strip()) for f in m.group(1).split(";") if f.strip()] == ["double mrSize", "int patchSize", "double mean[3]"]
    modsx.lib().modsx_default_caffe_params(None)                 # a null pointer is ignored
    q = modsx.caffe_params(mr_size=7.5, patch_size=65, mean=(1, 2, 3))
    assert (q.mrSize, q.patchSize, list(q.mean)) == (7.5, 65, [1.0, 2.0, 3.0])


@pytest.mark.parametrize("P", Cs.PATCH_SIZES)
def test_jobs_equal_the_model_bit_for_bit(modsx, oracle, P):
    for mr in (Cs.MR_SIZE, 1.0, 20.9, 0.0):
        for name, (rows, cols) in Cs.IMAGES.items():
            regs = Cs.regions(name, P, mr)
            got = modsx.caffe_jobs(regs, modsx.caffe_params(mr_size=mr, patch_size=P), rows, cols)
            want = M.jobs(regs, mr, P)
            for f in modsx.CAFFE_JOB_FIELDS:
                assert np.array_equal(u32(got[f]), u32(want[f])), (P, mr, name, f)
            assert np.array_equal(got["border"], M.border(want, rows, cols, P)), (P, mr, name)
            if mr == Cs.MR_SIZE:
                assert got["border"].any() and not got["border"].all()
    assert modsx.caffe_jobs(Cs.regions("a", P)[:0], modsx.caffe_params(patch_size=P), 48, 64)["border"].shape == (0,)


def test_geometry(modsx):
    for P in Cs.PATCH_SIZES:
        for n in Cs.COUNTS:
            g = modsx.caffe_geometry(n, P)
            assert g["workgroups"] == 8 * ((n + 7) // 8) >= n
            assert g["waves"] == (P + 63) // 64 and 64 * g["waves"] >= P           # one lane per patch row
            assert g["chunk_cols"] == min(P, 64) and g["chunks"] * g["chunk_cols"] >= P > (g["chunks"] - 1) * g["chunk_cols"]
            assert g["lds_stride"] >= g["chunk_cols"] and g["lds_stride"] % 4 == 0 and (g["lds_stride"] // 4) % 2 == 1
            assert g["lds_bytes_gray"] == g["lds_stride"] * P and g["lds_bytes_colour"] == 3 * g["lds_bytes_gray"] <= 64 * 1024
    assert modsx.caffe_geometry(1, 255)["lds_bytes_colour"] > 4 * modsx.caffe_geometry(1, 41)["lds_bytes_colour"]      # sized by P


def test_refusals_without_a_device(modsx):
    L = modsx.lib()
    regs = Cs.regions("a", 41)
    rp = regs.ctypes.data_as(C.c_void_p)
    buf = np.zeros(8 * len(regs), np.float32)
    bp = buf.ctypes.data_as(C.c_void_p)
    ok = modsx.caffe_params()
    bad = [modsx.caffe_params(patch_size=ps) for ps in (0, -1, 2, 40, 42, 256, 257)]
    bad += [modsx.caffe_params(mr_size=mr) for mr in (float("nan"), float("inf"), -float("inf"), -0.5, 1.0000001e6)]
    bad += [modsx.caffe_params(mean=m) for m in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, 2.0 ** 30 + 1), (-2.0 ** 30 - 1, 0, 0))]
    planes3 = (C.c_void_p * 3)(1, 1, 1)          # never dereferenced: every call below is refused before it looks at a plane
    for p in bad:
        assert L.modsx_caffe_jobs(rp, len(regs), C.byref(p), 48, 64, bp) == -1
        assert L.modsx_caffe_patches(None, planes3, 3, rp, len(regs), C.byref(p), bp, None) == -1
        assert L.modsx_caffe_patches_device(None, planes3, 3, rp, len(regs), C.byref(p), bp, None) == -1
        assert b"null argument" not in L.modsx_last_error()          # the parameters are refused first
    for ps in (2, 256):
        assert L.modsx_debug_caffe_geometry(1, ps, bp) == -1 and b"patchSize" in L.modsx_last_error()
    assert L.modsx_debug_caffe_geometry(-1, 41, bp) == -1 and L.modsx_debug_caffe_geometry(1, 41, None) == -1
    # the bounds themselves pass
    for p in (modsx.caffe_params(patch_size=1), modsx.caffe_params(patch_size=255), modsx.caffe_params(mr_size=0.0),
              modsx.caffe_params(mr_size=1e6), modsx.caffe_params(mean=(2.0 ** 30, -2.0 ** 30, 0))):
        assert L.modsx_caffe_jobs(rp, len(regs), C.byref(p), 48, 64, bp) == len(regs)
    # counts and pointers
    assert L.modsx_caffe_jobs(rp, -1, C.byref(ok), 48, 64, bp) == -1
    assert L.modsx_caffe_jobs(None, 1, C.byref(ok), 48, 64, bp) == -1
    assert L.modsx_caffe_jobs(rp, 1, C.byref(ok), 48, 64, None) == -1
    assert L.modsx_caffe_jobs(rp, 1, None, 48, 64, bp) == -1
    assert L.modsx_caffe_jobs(rp, 1, C.byref(ok), 1, 64, bp) == -1
    for fn in (L.modsx_caffe_patches, L.modsx_caffe_patches_device):
        assert fn(None, planes3, 3, rp, -1, C.byref(ok), bp, None) == -1
        assert fn(None, planes3, 3, None, 1, C.byref(ok), bp, None) == -1
        assert fn(None, planes3, 3, rp, 1, C.byref(ok), None, None) == -1
        assert fn(None, planes3, 3, rp, 1, None, bp, None) == -1
        for np_ in (0, 2, 4, -1):
            assert fn(None, planes3, np_, rp, 1, C.byref(ok), bp, None) == -1 and b"planes" in L.modsx_last_error()
        assert fn(None, None, 3, rp, 1, C.byref(ok), bp, None) == -1
        assert fn(None, (C.c_void_p * 3)(1, None, 1), 3, rp, 1, C.byref(ok), bp, None) == -1
        assert fn(None, planes3, 3, rp, 1, C.byref(ok), bp, None) == -1 and b"null argument: ctx" in L.modsx_last_error()
    assert L.modsx_caffe_patches_device(None, planes3, 3, rp, 1, C.byref(ok), C.c_void_p(bp.value + 2), None) == -1
    assert b"aligned" in L.modsx_last_error()
    # the norms
    for fn in (L.modsx_caffe_norm_rows, L.modsx_caffe_norm_rows_device):
        assert fn(None, bp, -1, 4, 0, bp) == -1
        for dim in (0, -4, 4097):
            assert fn(None, bp, 1, dim, 0, bp) == -1 and b"dim" in L.modsx_last_error()
        for norm in (-1, 4):
            assert fn(None, bp, 1, 4, norm, bp) == -1 and b"norm" in L.modsx_last_error()
        assert fn(None, None, 1, 4, 0, bp) == -1 and fn(None, bp, 1, 4, 0, None) == -1
        assert fn(None, bp, 1, 4, 0, bp) == -1 and b"null argument: ctx" in L.modsx_last_error()
    assert L.modsx_caffe_norm_rows_device(None, C.c_void_p(bp.value + 1), 1, 4, 0, bp) == -1
    assert L.modsx_caffe_norm_rows_device(None, bp, 1, 4, 0, C.c_void_p(bp.value + 2)) == -1
    assert L.modsx_caffe_counters(None, bp, 4) == -1
    # the device append: what the host append refuses before it touches the context
    for fn in (L.modsx_rep_append_f32_device, L.modsx_rep_append_f32):
        assert fn(None, None, modsx.DET_HESSIAN, modsx.DESC_CAFFE, rp, bp, 4, 1) == -1
    assert b"modsx_rep_append_f32:" in L.modsx_last_error()
