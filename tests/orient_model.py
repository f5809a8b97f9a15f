"""numpy restatement of EstimateDominantAnglesFunctor (oracle/oracle_describe.cpp: dominant_angles), for INTROSPECTION: the
reference of the GPU tests is the oracle; this model says why a patch gives the answer it gives -- which atan2LUT table entry and
which histogram bin every mask pixel reaches, how many votes a bin gets, the raw / smoothed / folded histograms, the threshold and
the peaks before the cut -- so that tests/test_orient_cases_cpu.py can prove what tests/orient_cases.py claims.  No GPU in here.

The arithmetic is f32 in the oracle's order: gradients and sqrtf per pixel, mag * mask, per-bin running sums in raster order,
six passes of (prev + cur) + next, thresh = (float)((double)max * th), the Half fold, strict peaks, the parabola and the angle.
The angle of a gradient comes from oracle.atan_lut() with the sign / octant code and the table index of atan2LUTff
(code = (x > 0) << 2 | (y > 0) << 1 | (|x| > |y|), idx = (int)(255 * small / big)); expf of the mask is libm's, as in the oracle.

MUTATIONS names the deliberate mistakes `mut=` accepts: each one must change the answer of a planted case (the sensitivity proof).
"""
import ctypes as C
import ctypes.util

import numpy as np

PS, HALF, BINS = 41, 20, 36
NVOTERS = 1245                      # pixels under the mask
F = np.float32
PIf = F(np.pi)
PI_2f = F(np.pi / 2)
MUTATIONS = ("peak_ge", "thresh_gt", "mag_ge", "reverse_raster", "smooth_right_first", "five_passes", "bin36_to_0", "bin36_to_35",
             "cut_largest", "bin_floor")

_mask = None
_lut = None


_libm = None


def libm():
    """the C library's f32 expf / cosf / sinf: what the oracle and the library's host code call (numpy's own f32 routines may
    round differently)"""
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for f in (_libm.expf, _libm.cosf, _libm.sinf):
            f.restype = C.c_float
            f.argtypes = [C.c_float]
    return _libm


def circular_gauss_mask():
    """computeCircularGaussMask(41, 41 / 3.0f) -> [41, 41] f32 (0 outside the disc of radius 20)"""
    global _mask
    if _mask is None:
        sigma = F(PS) / F(3.0)
        sigma2 = F(2) * sigma * sigma
        r2 = F(HALF * HALF)
        m = np.zeros((PS, PS), F)
        for i in range(PS):
            for j in range(PS):
                disq = F((i - HALF) * (i - HALF) + (j - HALF) * (j - HALF))
                if disq < r2:
                    m[i, j] = libm().expf(-disq / sigma2)
        _mask = m
    return _mask


def voting_list():
    """(rows, cols) of the mask pixels in raster order: the kernel's voting list before its padding"""
    r, c = np.nonzero(circular_gauss_mask() > 0)
    return r, c


def lut(oracle):
    global _lut
    if _lut is None:
        _lut = oracle.atan_lut()
    return _lut


def atan_case(y, x):
    """atan2LUTff's branch and table index for f32 arrays -> (code, idx, special); idx is clamped like the kernel's (the reference
    never leaves 0 .. 255 for finite input: small <= big)"""
    y, x = np.asarray(y, F), np.asarray(x, F)
    ax, ay = np.abs(x), np.abs(y)
    xp, yp, big = x > 0, y > 0, ax > ay
    num, den = np.where(big, ay, ax), np.where(big, ax, ay)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = (F(255) * num) / den
    q = np.where(np.isnan(q), F(0), q)                      # x = y = 0: the special case, the index is not used
    idx = np.clip(np.trunc(q), 0, 255).astype(np.int32)
    code = (xp.astype(np.int32) << 2) | (yp.astype(np.int32) << 1) | big.astype(np.int32)
    special = ~xp & ~yp & ~big & (x == 0)
    return code, idx, special


def angle_of_case(L, code, idx, special=None):
    """the f32 angle atan2LUTff returns in branch `code` at table index `idx` (0 in the special case)"""
    code, idx = np.asarray(code), np.asarray(idx)
    xp, yp, big = (code & 4) != 0, (code & 2) != 0, (code & 1) != 0
    Lv = np.asarray(L, np.float64)[idx]
    neg = np.where(xp, np.where(yp, ~big, big), np.where(yp, big, ~big))
    sL = np.where(neg, -Lv, Lv)
    c = np.where(big, np.where(xp, 0.0, np.where(yp, np.float64(PIf), -np.float64(PIf))),
                 np.where(yp, np.float64(PI_2f), -np.float64(PI_2f)))
    out = np.where(big & xp, sL.astype(F), (c + sL).astype(F)).astype(F)
    if special is not None:
        out = np.where(special, F(0), out)
    return out


def bin_of_angle(ori, floor=False):
    """(int)(36 * (ori / pi + 1) / 2), f32"""
    v = (F(BINS) * (np.asarray(ori, F) / PIf + F(1.0))) / F(2.0)
    return (np.floor(v) if floor else np.trunc(v)).astype(np.int32)


def analyse(oracle, patches, mut=()):
    """patches [N, 41, 41] f32 -> dict:
    bin [N, 41, 41] int (-1: no vote), code / idx / special [N, 41, 41] (of every pixel's gradient; meaningful where bin >= 0),
    mag [N, 41, 41] f32, votes [N, 37] int, raw [N, 37] f32 (slot 36 is the reference's unread one)."""
    p = np.ascontiguousarray(patches, F).reshape(-1, PS, PS)
    n = len(p)
    mask = circular_gauss_mask()
    xg = np.zeros_like(p)
    yg = np.zeros_like(p)
    xg[:, 1:-1, 1:-1] = p[:, 1:-1, 2:] - p[:, 1:-1, :-2]
    yg[:, 1:-1, 1:-1] = p[:, 2:, 1:-1] - p[:, :-2, 1:-1]
    mag = np.sqrt(xg * xg + yg * yg)
    code, idx, special = atan_case(yg, xg)
    ori = angle_of_case(lut(oracle), code, idx, special)
    b = bin_of_angle(ori, floor="bin_floor" in mut)
    if "bin36_to_0" in mut:
        b = np.where(b == BINS, 0, b)
    if "bin36_to_35" in mut:
        b = np.where(b == BINS, BINS - 1, b)
    votes_px = (mask[None] > 0) & ((mag >= F(1.0)) if "mag_ge" in mut else (mag > F(1.0)))
    votes_px[:, 0, :] = votes_px[:, -1, :] = False
    votes_px[:, :, 0] = votes_px[:, :, -1] = False
    b = np.where(votes_px, b, -1)
    w = (mag * mask[None]).reshape(n, -1)
    bf = b.reshape(n, -1)
    if "reverse_raster" in mut:
        w, bf = w[:, ::-1], bf[:, ::-1]
    raw = np.zeros((n, BINS + 1), F)
    votes = np.zeros((n, BINS + 1), np.int64)
    for k in range(BINS + 1):
        sel = bf == k
        votes[:, k] = sel.sum(1)
        # x + 0 = x: the running sum over all pixels with the others' weights zeroed is the bin's own running sum
        raw[:, k] = np.cumsum(np.where(sel, w, F(0)), axis=1, dtype=F)[:, -1]
    return dict(bin=b, code=code, idx=idx, special=special, mag=mag, votes=votes, raw=raw)


def peaks(raw, half=0, th=0.8, mut=()):
    """raw [N, >= 36] f32 -> dict(smoothed, thresh, folded, peak [N, 36] bool (before the cut), angle [N, 36] f32 (where peak))"""
    h = np.ascontiguousarray(np.asarray(raw, F)[:, :BINS])
    for _ in range(5 if "five_passes" in mut else 6):
        prev, nxt = np.roll(h, 1, axis=1), np.roll(h, -1, axis=1)
        h = (prev + (h + nxt)) if "smooth_right_first" in mut else ((prev + h) + nxt)
    smoothed = h
    mx = np.maximum(h.max(1), F(0))
    thresh = (mx.astype(np.float64) * float(th)).astype(F)
    if half:
        h = h.copy()
        h[:, :BINS // 2] = h[:, :BINS // 2] + h[:, BINS // 2:]
        h[:, BINS // 2:] = 0
    a, c = np.roll(h, 1, axis=1), np.roll(h, -1, axis=1)
    t = thresh[:, None]
    over = (h > t) if "thresh_gt" in mut else (h >= t)
    pk = over & ((h >= a) & (h >= c) if "peak_ge" in mut else (h > a) & (h > c))
    with np.errstate(invalid="ignore", divide="ignore"):
        pp = ((a - c) / ((a - F(2.0) * h) + c)) / F(2.0)
        bidx = np.arange(BINS, dtype=F)[None]
        ang = ((F(2.0) * PIf) * ((bidx + F(0.5)) + pp)) / F(BINS) - PIf
    return dict(smoothed=smoothed, thresh=thresh, folded=h, peak=pk, angle=ang.astype(F))


def cut(pk, max_angles, mut=()):
    """the angles of one patch: the first min(max_angles, #peaks) peaks in bin order (-1: all, 0: none)"""
    bins = np.nonzero(pk["peak"])[0]
    if max_angles == 0:
        return bins[:0]
    if max_angles > 0 and len(bins) > max_angles:
        if "cut_largest" in mut:
            keep = np.sort(bins[np.argsort(-pk["folded"][bins], kind="stable")[:max_angles]])
        else:
            keep = bins[:max_angles]
        return keep
    return bins


def dominant_angles_batch(oracle, patches, half=0, th=0.8, max_angles=-1, mut=(), analysis=None):
    """-> (list of f32 angle arrays, report): report = analyse() + peaks() of the batch"""
    rep = dict(analysis if analysis is not None and not (set(mut) & _ANALYSE_MUT) else analyse(oracle, patches, mut))
    pk = peaks(rep["raw"], half, th, mut)
    rep.update(pk)
    out = []
    for i in range(len(rep["raw"])):
        one = dict(peak=pk["peak"][i], folded=pk["folded"][i])
        out.append(pk["angle"][i][cut(one, max_angles, mut)].astype(F))
    return out, rep


_ANALYSE_MUT = {"mag_ge", "reverse_raster", "bin36_to_0", "bin36_to_35", "bin_floor"}


def dominant_angles(oracle, patch, half=0, th=0.8, max_angles=-1, mut=()):
    """one patch -> (angles f32, report with the leading axis removed)"""
    a, rep = dominant_angles_batch(oracle, np.asarray(patch, F)[None], half, th, max_angles, mut)
    return a[0], {k: v[0] for k, v in rep.items()}
