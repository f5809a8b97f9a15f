"""CPU: the C boundary of the external affine adaptation (include/modsx.h: DetectAffineShape on a caller's regions) -- the
argument lists of the new symbols as the header declares them, the defaults of AffineShapeParams(), every refusal that needs
no device, and the results that need no launch (n = 0, maxIterations <= 0).  Parameters and regions are checked before the
context is looked at, so the entries are called here without one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1

SYMBOLS = {
    "modsx_default_affshape_params": "modsx_affshape_params *p",
    "modsx_detect_affine_shape": "modsx_ctx *ctx, const modsx_image *img, const modsx_region *in, int n, "
                                 "const modsx_affshape_params *par, modsx_region **out",
    "modsx_detect_affine_shape_batch": "modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_region *in, "
                                       "const int *counts, const modsx_affshape_params *par, modsx_region **out, int *out_counts",
    "modsx_debug_affine_shape": "modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_region *in, const int *counts, "
                                "const modsx_affshape_params *par, int variant, unsigned char *border, float *u, int *ok, int *iters, "
                                "int *geometry",
    "modsx_affshape_jobs": "const modsx_region *in, int n, int cols, int rows, float *ratio, int *res, unsigned char *border",
    "modsx_affshape_counters": "modsx_ctx *ctx, long *out, int n",
}


def _region(modsx, n=1, s=1.6):
    r = np.zeros(n, modsx.REGION)
    r["det_kp"]["x"], r["det_kp"]["y"], r["det_kp"]["s"] = 20.0, 20.0, s
    r["det_kp"]["a11"], r["det_kp"]["a22"] = 1.0, 1.0
    return r


def _detect(modsx, regs, par, n=None):
    """modsx_detect_affine_shape without a context or an image -> (return value, error text)"""
    out = C.c_void_p()
    rc = modsx.lib().modsx_detect_affine_shape(None, None, regs.ctypes.data_as(C.c_void_p), len(regs) if n is None else n,
                                               C.byref(par) if par is not None else None, C.byref(out))
    if out:
        modsx.lib().modsx_free(out)
    return rc, modsx.lib().modsx_last_error().decode()


def test_declared_argument_lists(modsx):
    hdr = open(os.path.join(ROOT, "include", "modsx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, args in SYMBOLS.items():
        m = re.search(r"\b(?:int|void)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        assert " ".join(m.group(1).split()) == " ".join(args.split()), name
        assert name in modsx.EXPORTS and hasattr(modsx.lib(), name)
    m = re.search(r"typedef struct modsx_affshape_params \{(.*?)\} modsx_affshape_params;", hdr, re.S)
    fields = re.findall(r"\b(int|float)\s+(\w+)\s*;", m.group(1))
    assert fields == [("int", "maxIterations"), ("int", "smmWindowSize"), ("float", "convergenceThreshold"), ("int", "affBmbrgMethod")]
    assert [(f[1], f[0]) for f in fields] == [(n, "int" if t is C.c_int else "float") for n, t in modsx.AffShapeParams._fields_]
    assert C.sizeof(modsx.AffShapeParams) == 16


def test_defaults_are_those_of_affine_shape_params(modsx):
    p = modsx.default_affshape_params()      # AffineShapeParams(), detectors/affinedetectors/affine.h:52-63
    assert (p.maxIterations, p.smmWindowSize, p.affBmbrgMethod) == (16, 19, 0)
    assert np.float32(p.convergenceThreshold) == np.float32(0.05)
    q = modsx.default_affshape_params(maxIterations=3, smmWindowSize=11)
    assert (q.maxIterations, q.smmWindowSize) == (3, 11)
    with pytest.raises(AttributeError):
        modsx.default_affshape_params(initialSigma=1.0)       # no such parameter: the function's own constant is used


@pytest.mark.parametrize("W", [-1, 0, 1, 2, 4, 18, 20, 21, 41])
def test_window_sizes_refused(modsx, W):
    rc, err = _detect(modsx, _region(modsx), modsx.default_affshape_params(smmWindowSize=W))
    assert rc == ERR_ARG and "smmWindowSize" in err


def test_hessian_method_refused(modsx):
    rc, err = _detect(modsx, _region(modsx), modsx.default_affshape_params(affBmbrgMethod=1))
    assert rc == ERR_ARG and "AFF_BMBRG_HESSIAN" in err


@pytest.mark.parametrize("field", ["x", "y", "s", "a11", "a12", "a21", "a22"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_regions_refused(modsx, field, value):
    regs = _region(modsx, 3)
    regs["det_kp"][field][1] = value
    rc, err = _detect(modsx, regs, modsx.default_affshape_params())
    assert rc == ERR_ARG and "region 1" in err and "non-finite" in err
    with pytest.raises(RuntimeError, match="non-finite"):
        modsx.affshape_jobs(regs, 64, 48)
    # also when nothing would be launched
    rc, _ = _detect(modsx, regs, modsx.default_affshape_params(maxIterations=0))
    assert rc == ERR_ARG


def test_window_argument_outside_int_refused(modsx):
    """|10 * ratio| >= 2^31: the reference's double -> int conversion is undefined there"""
    sigma = np.float64(np.float32(1.6))
    edge = 2.0 ** 31 / 10.0 * sigma
    for s, ok in ((edge * 0.999, True), (-edge * 0.999, True), (edge * 1.001, False), (-edge * 1.001, False), (1e300, False)):
        regs = _region(modsx, 2, s=1.6)
        regs["det_kp"]["s"][1] = s
        if ok:
            got = modsx.affshape_jobs(regs, 64, 48)
            assert abs(int(got["res"][1])) > 2 ** 31 * 0.99 and got["border"][1]
        else:
            with pytest.raises(RuntimeError, match="2\\^31"):
                modsx.affshape_jobs(regs, 64, 48)
            rc, err = _detect(modsx, regs, modsx.default_affshape_params())
            assert rc == ERR_ARG and "region 1" in err


@pytest.mark.parametrize("cols,rows", [(3, 40), (40, 3), (0, 0), (-5, 40)])
def test_small_images_refused(modsx, cols, rows):
    with pytest.raises(RuntimeError, match="4 x 4"):
        modsx.affshape_jobs(_region(modsx), cols, rows)
    modsx.affshape_jobs(_region(modsx), 4, 4)


def test_bad_counts_and_null_pointers(modsx):
    par = modsx.default_affshape_params()
    rc, _ = _detect(modsx, _region(modsx), par, n=-1)
    assert rc == ERR_ARG
    rc, err = _detect(modsx, _region(modsx), None)
    assert rc == ERR_ARG and "par" in err
    assert modsx.lib().modsx_detect_affine_shape(None, None, None, 1, C.byref(par), C.byref(C.c_void_p())) == ERR_ARG    # regions missing
    assert modsx.lib().modsx_detect_affine_shape(None, None, None, 0, C.byref(par), None) == ERR_ARG                      # out missing
    # a valid call still needs a context and an image
    rc, err = _detect(modsx, _region(modsx), par)
    assert rc == ERR_ARG and "ctx" in err
    assert modsx.lib().modsx_affshape_counters(None, None, 0) == ERR_ARG
    assert modsx.lib().modsx_affshape_jobs(None, 2, 64, 48, None, None, None) == ERR_ARG
    assert modsx.lib().modsx_affshape_jobs(None, 0, 64, 48, None, None, None) == 0


def test_no_regions_and_no_iterations_give_an_empty_list(modsx):
    par = modsx.default_affshape_params()
    out = C.c_void_p()
    assert modsx.lib().modsx_detect_affine_shape(None, None, None, 0, C.byref(par), C.byref(out)) == 0
    assert out.value                                   # an empty malloc'd array, released like any other
    modsx.lib().modsx_free(out)
    regs = _region(modsx, 5)
    for iters in (0, -3):
        out = C.c_void_p()
        p0 = modsx.default_affshape_params(maxIterations=iters)
        assert modsx.lib().modsx_detect_affine_shape(None, None, regs.ctypes.data_as(C.c_void_p), 5, C.byref(p0), C.byref(out)) == 0
        assert out.value
        modsx.lib().modsx_free(out)
    # the batch form: counts are reported as zeros
    counts, out_counts = np.array([2, 0, 3], np.int32), np.full(3, 7, np.int32)
    out = C.c_void_p()
    p0 = modsx.default_affshape_params(maxIterations=0)
    assert modsx.lib().modsx_detect_affine_shape_batch(None, None, 3, regs.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                       C.byref(p0), C.byref(out), out_counts.ctypes.data_as(C.c_void_p)) == 0
    assert (out_counts == 0).all()
    modsx.lib().modsx_free(out)
    out = C.c_void_p()
    assert modsx.lib().modsx_detect_affine_shape_batch(None, None, 0, None, None, C.byref(par), C.byref(out), None) == 0
    modsx.lib().modsx_free(out)


def test_jobs_of_simple_regions(modsx):
    regs = _region(modsx, 4)
    regs["det_kp"]["s"] = [1.6, float(np.float32(1.6)), -float(np.float32(1.6)) * 0.75, 0.0]
    got = modsx.affshape_jobs(regs, 64, 48)
    # 1.6 (a double) / 1.6f is just below 1: the ratio rounds to 1, the f32 number 1.6f gives exactly 1
    assert got["ratio"].tolist() == [1.0, 1.0, -0.75, 0.0] and got["res"].tolist() == [10, 10, -7, 0]
    assert not got["border"].any()
