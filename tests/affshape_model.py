"""DetectAffineShape (synth-detection.cpp:922-1074) restated from the oracle's parts, for tests/test_affshape_cases_cpu.py and
tests/test_gpu_affshape.py.  No GPU in here, and nothing of the library under test.

Per region:
  1. ratio = np.float32(np.float64(s) / np.float64(np.float32(1.6)))          (:950, s a double, initialSigma a const float)
  2. res   = int(10.0 * float64(ratio)), truncated toward zero                  (:961, the int parameter of the border test)
  3. border = oracle.interpolate_check_borders(cols, rows, f32 x, f32 y, f32 a11 .. a22, res)          (:954-964)
  4. the regions that pass run oracle.find_affine_shape_batch on the image as the plane with (x, y, s, pixelDistance = 1) and
     affInitialSigma = 1.6: the loop body of DetectAffineShape is that of findAffineShape line for line, and it starts from the
     identity.
The oracle forms its ratio as the f32 quotient s / (1.6f * 1.0f).  For an s that is an f32 number that equals step 1 (an f64
quotient of two f32 numbers, rounded to f32, is the correctly rounded f32 quotient: 53 >= 2 * 24 + 2 bits); for any other s it
need not, so the model refuses such regions -- `assert_f32_scales`.  Non-f32 scales are checked on the host alone
(test_affshape_cases_cpu.py against `ratio_res`).

Output of `run`: the regions with reason == 0 in input order with det_kp.a11 .. a22 = the f32 shape widened to double, and the
per-INPUT-region report dict(border, ratio, res, u, ok, iters, reason, touch) -- u identity, ok 0, iters -1, reason -1, touch 0
for a border-refused region.
"""
import numpy as np

SIGMA = np.float32(1.6)


def ratio_res(s):
    """-> (ratio f32 [n], res i32 [n]) of scales s (any doubles)"""
    s = np.asarray(s, np.float64)
    ratio = (s / np.float64(SIGMA)).astype(np.float32)
    w = 10.0 * ratio.astype(np.float64)
    assert (np.abs(w) < 2.0 ** 31).all()
    return ratio, np.trunc(w).astype(np.int32)


def assert_f32_scales(regs):
    s = regs["det_kp"]["s"]
    assert (s.astype(np.float32).astype(np.float64) == s).all(), "the oracle path of the model takes f32-representable scales only"


def border_test(oracle, regs, rows, cols):
    """the up-front interpolateCheckBorders with the region's own matrix rounded to f32 -> (border bool [n], ratio, res)"""
    k = regs["det_kp"]
    ratio, res = ratio_res(k["s"])
    f = lambda a: a.astype(np.float32).astype(np.float64)         # noqa: E731  (the tuples travel as Python floats: exact)
    t = np.stack([np.full(len(regs), cols, np.float64), np.full(len(regs), rows, np.float64), f(k["x"]), f(k["y"]), f(k["a11"]),
                  f(k["a12"]), f(k["a21"]), f(k["a22"]), res.astype(np.float64)], 1) if len(regs) else np.zeros((0, 9))
    return oracle.interpolate_check_borders(t), ratio, res


def run(oracle, img, regs, **params):
    """DetectAffineShape(regs, img) -> (out regions, report); params: maxIterations, convergenceThreshold, smmWindowSize"""
    img = np.ascontiguousarray(img, np.float32)
    n = len(regs)
    assert_f32_scales(regs)
    border, ratio, res = border_test(oracle, regs, img.shape[0], img.shape[1])
    rep = dict(border=border, ratio=ratio, res=res, u=np.tile(np.array([1, 0, 0, 1], np.float32), (n, 1)), ok=np.zeros(n, np.int32),
               iters=np.full(n, -1, np.int32), reason=np.full(n, -1, np.int32), touch=np.zeros(n, np.int32))
    idx = np.nonzero(~border)[0]
    if len(idx):
        k = regs["det_kp"][idx]
        xyspd = np.stack([k["x"].astype(np.float32), k["y"].astype(np.float32), k["s"].astype(np.float32),
                          np.ones(len(idx), np.float32)], 1)
        par = oracle.default_params(affInitialSigma=float(SIGMA), **params)
        assert np.float32(par.affInitialSigma) == SIGMA
        r = oracle.find_affine_shape_batch([img], np.zeros(len(idx), np.int32), xyspd, par)
        for f in ("u", "ok", "iters", "reason", "touch"):
            rep[f][idx] = r[f]
    if params.get("maxIterations", 16) <= 0:
        keep = np.zeros(n, bool)
    else:
        keep = rep["reason"] == 0
        assert np.array_equal(keep, rep["ok"] == 1)
    out = regs[keep].copy()
    for i, f in enumerate(("a11", "a12", "a21", "a22")):
        out["det_kp"][f] = rep["u"][keep, i].astype(np.float64)
    for v in rep.values():
        v.setflags(write=False)
    return out, rep
