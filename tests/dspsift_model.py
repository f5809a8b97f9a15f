"""A numpy restatement of what the reference's "DSPSIFT" branch (imagerepresentation.cpp:1547-1598) computes from a normalised
41 x 41 patch on: the raw SIFT histogram of SIFTDescriptor{useRootSIFT = false, doNorm = false} (matching/siftdesc.cpp:22-131,
290-326, 401-442), the f32 pooling over measurement sizes, and SIFTnorm(std::vector<float>&) (siftdesc.cpp:160-185, 263-278).
tests/test_dspsift_model_cpu.py ties it bit for bit to the compiled reference's recorded results (tests/golden/dspsift_ref.npz,
written by tools/make_dspsift_fixture.py) and, through the f64 norms restated at the end, to oracle.describe_patch.

Number formats follow the reference statement by statement: what is a float there is np.float32 here, what is promoted to double
there is computed in np.float64 and rounded where the reference assigns it to a float.  numpy's f32 / f64 add, multiply, divide
and sqrt are the IEEE operations; the angle look-up is the oracle's atan2lut; the mask's exponential is libm's expf, which the
oracle uses too (numpy's exp is another implementation)."""
import ctypes as C
import ctypes.util
import functools

import numpy as np

PS, NPX, SPATIAL, ORI, DIM = 41, 41 * 41, 4, 8, 128
TWO_PI = 6.28318530718          # M_PI_DOUBLED, siftdesc.cpp:18
f32, f64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _libm():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.expf.restype = C.c_float
    m.expf.argtypes = [C.c_float]
    return m


@functools.lru_cache(maxsize=None)
def mask():
    """computeCircularGaussMask(mask, 0), detectors/helpers.cpp:442-461: [41][41] f32"""
    half = PS >> 1
    r2 = f32(half * half)
    sigma2 = f32(0.9) * r2
    out = np.zeros((PS, PS), f32)
    for i in range(PS):
        for j in range(PS):
            disq = f32((i - half) * (i - half) + (j - half) * (j - half))
            out[i, j] = f32(_libm().expf(C.c_float(float(-disq / sigma2)))) if disq < r2 else f32(0)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bins_and_weights():
    """precomputeBinsAndWeights, siftdesc.cpp:22-71: (bin0, bin1) int, already times orientationBins; (w0, w1) f64"""
    half = PS >> 1
    step = f32(SPATIAL + 1) / f32(2 * half)
    bin0, bin1 = np.zeros(PS, np.int64), np.zeros(PS, np.int64)
    w0, w1 = np.zeros(PS, f64), np.zeros(PS, f64)
    for i in range(PS):
        x = step * f32(i)
        xi = int(x)
        bin0[i], bin1[i] = xi - 1, xi
        w1[i] = f64(x - f32(xi))                  # x - xi in float, stored to a double
        w0[i] = f64(1.0) - w1[i]                  # 1.0f - w1[i]: w1 is a double there
        if bin0[i] < 0:
            bin0[i], w0[i] = 0, 0
        if bin0[i] >= SPATIAL:
            bin0[i], w0[i] = SPATIAL - 1, 0
        if bin1[i] < 0:
            bin1[i], w1[i] = 0, 0
        if bin1[i] >= SPATIAL:
            bin1[i], w1[i] = SPATIAL - 1, 0
    return bin0 * ORI, bin1 * ORI, w0, w1


def gradients(patch):
    """computeSiftDescriptor's loop, siftdesc.cpp:301-325: (grad, ori) [41][41] f32, one-sided differences on the frame"""
    from oracle import pyoracle as O
    p = np.ascontiguousarray(patch, f32).reshape(PS, PS)
    xg = np.empty((PS, PS), f32)
    yg = np.empty((PS, PS), f32)
    xg[:, 1:-1] = p[:, 2:] - p[:, :-2]
    xg[:, 0] = p[:, 1] - p[:, 0]
    xg[:, -1] = p[:, -1] - p[:, -2]
    yg[1:-1] = p[2:] - p[:-2]
    yg[0] = p[1] - p[0]
    yg[-1] = p[-1] - p[-2]
    grad = np.sqrt(xg * xg + yg * yg)             # f32 products, f32 sum, correctly rounded root
    ori = np.array([O.atan2lut(float(y), float(x)) for y, x in zip(yg.reshape(-1), xg.reshape(-1))], f32).reshape(PS, PS)
    return grad, ori


def sample_terms(patch):
    """samplePatch, siftdesc.cpp:73-131, unrolled: (bins [1681 * 8], terms [1681 * 8] f64) in the order of the reference's adds,
    the adds behind a failed `val > 0` left out"""
    grad, ori = gradients(patch)
    b0, b1, w0, w1 = bins_and_weights()
    r, c = (a.reshape(-1) for a in np.mgrid[0:PS, 0:PS])
    # float val = float(magnLess) * 1.0 + (1.0 - float(magnLess)) * mask * grad: f64 throughout, rounded once
    val = (f64(0.0) + (f64(1.0) * mask().reshape(-1).astype(f64)) * grad.reshape(-1).astype(f64)).astype(f32)
    wc0 = (w0[c] * val.astype(f64)).astype(f32)
    wc1 = (w1[c] * val.astype(f64)).astype(f32)
    wr0, wr1 = w0[r].astype(f32), w1[r].astype(f32)
    o = ((f64(8.0) * (ori.reshape(-1).astype(f64) + TWO_PI)) / TWO_PI).astype(f32)
    bo0 = o.astype(np.int64)                      # (int)o: o > 0
    wo1 = o - bo0.astype(f32)
    bo0 %= ORI
    bo1 = (bo0 + 1) % ORI
    wo0 = f32(1.0) - wo1
    br0, br1, bc0, bc1 = SPATIAL * b0[r], SPATIAL * b1[r], b0[c], b1[c]
    bins, terms = [], []
    for wr, br in ((wr0, br0), (wr1, br1)):
        for wc, bc in ((wc0, bc0), (wc1, bc1)):
            v = wr * wc                            # f32
            ok = v > 0
            for wo, bo in ((wo0, bo0), (wo1, bo1)):
                bins.append(np.where(ok, br + bc + bo, -1))
                terms.append((v * wo).astype(f64))      # the f32 product, promoted for the add
    bins = np.stack(bins, 1).reshape(-1)           # pixel after pixel in raster order, the eight adds of a pixel in theirs
    terms = np.stack(terms, 1).reshape(-1)
    keep = bins >= 0
    return bins[keep], terms[keep]


def histogram_f64(patch):
    """vec[128] of sample(false): every bin adds its terms in the reference's order (np.add.at is unbuffered and in order)"""
    bins, terms = sample_terms(patch)
    vec = np.zeros(DIM, f64)
    np.add.at(vec, bins, terms)
    return vec


def raw(patch):
    """the functor's output with doNorm = false: desc[i] = (float)vec[i], siftdesc.cpp:436-440"""
    return histogram_f64(patch).astype(f32)


def pool(hists, order=None):
    """acc = hist_0, then acc += hist_k in f32 (imagerepresentation.cpp:1568-1590).  hists: [scales][n][128] or [scales][128];
    order: another order of the scales, for the tests that show the order matters"""
    hists = np.asarray(hists, f32)
    idx = list(range(len(hists))) if order is None else list(order)
    acc = hists[idx[0]].copy()
    for k in idx[1:]:
        acc = acc + hists[k]
    return acc


def _normalize_f32(v, len_order=None):
    """normalize(std::vector<float>&), siftdesc.cpp:160-185, on rows [n][128]"""
    sq = v * v
    g = ((sq[:, 0::4] + sq[:, 1::4]) + sq[:, 2::4]) + sq[:, 3::4]
    ln = np.zeros(len(v), f32)
    for i in (range(32) if len_order is None else len_order):
        ln = ln + g[:, i]
    ln = np.sqrt(ln)
    fac = f64(1.0) / ln.astype(f64)
    return v * fac.astype(f32)[:, None]


def sift_norm_f32(rows, max_bin=0.2, len_order=None, info=None):
    """SIFTnorm(std::vector<float>&), siftdesc.cpp:263-278, on rows [n][128] (or one row) -> the same shape, f32 holding 0..255.
    A NaN converts to INT_MIN in the reference's x86-64 build and the clamp makes it 0.  info (a dict, optional) receives
    `clipped` [n] bool and `t` [n][128] f64 = (double)(512.0f * v) + 0.5 before the truncation."""
    rows = np.asarray(rows, f32)
    one = rows.ndim == 1
    v = rows.reshape(-1, DIM).copy()
    with np.errstate(all="ignore"):
        v = _normalize_f32(v, len_order)
        over = v.astype(f64) > f64(max_bin)
        v = np.where(over, f32(max_bin), v)
        changed = over.any(1)
        if changed.any():
            v[changed] = _normalize_f32(v[changed], len_order)
        t = (f32(512.0) * v).astype(f64) + 0.5
        b = np.where(np.isnan(t), 0.0, np.trunc(t))
    out = np.clip(b, 0.0, 255.0).astype(f32)
    if info is not None:
        info["clipped"], info["t"] = changed, t
    return out[0] if one else out


def mr_sizes(mr_size, num_scales, start_coef, end_coef):
    """curr_mrSize of imagerepresentation.cpp:1558-1559 for dsp_idx = 0 .. num_scales, in f64 as written"""
    return [f64(mr_size) * (f64(start_coef) + f64(k) * (f64(end_coef) - f64(start_coef)) / f64(num_scales)) for k in range(num_scales + 1)]


def dspsift(patches_per_scale, max_bin=0.2):
    """patches_per_scale: [scales][n] normalised patches -> [n][128] f32, the DSPSIFT descriptors"""
    hists = [[raw(p) for p in scale] for scale in patches_per_scale]
    return sift_norm_f32(pool(hists), max_bin)


# ---- the f64 norms of SIFTDescriptor::operator() (siftdesc.cpp:133-158, 199-221, 247-262, 411-435), restated for the tie to
# oracle.describe_patch: types 0 SIFT, 1 RootSIFT, 2 HalfSIFT, 3 HalfRootSIFT
def _normalize_f64(v):
    ln = f64(0.0)
    for i in range(0, len(v), 4):
        ln = ln + (((v[i] * v[i] + v[i + 1] * v[i + 1]) + v[i + 2] * v[i + 2]) + v[i + 3] * v[i + 3])
    return v * (f64(1.0) / np.sqrt(ln))


def describe_f64(vec, desc_type, max_bin=0.2):
    v = np.asarray(vec, f64).copy()
    if desc_type >= 2:
        v = (v.reshape(16, 2, 4)[:, 0] + v.reshape(16, 2, 4)[:, 1]).reshape(-1)
    with np.errstate(all="ignore"):
        v = _normalize_f64(v)
        over = v > f64(max_bin)
        if over.any():
            v = _normalize_f64(np.where(over, f64(max_bin), v))
        if desc_type & 1:
            s = f64(0.0)
            for x in v:
                s = s + abs(x)
            v = np.sqrt(v / s)
            t = f64(512.0) * v + 0.5
        else:
            t = f64(f32(512.0)) * v + 0.5
        b = np.clip(np.where(np.isnan(t), 0.0, np.trunc(t)), 0.0, 255.0)
    out = np.zeros(DIM, f32)
    out[:len(b)] = b
    return out
