"""A numpy / Python restatement of the reference's LIOP descriptor (LIOPDescriptor::operator(), matching/liopdesc.hpp:55-63 ->
vl_liopdesc_new_basic + vl_liopdesc_process, vlfeat/vl/liop.c:320-411, 440-555) for the 41 x 41 patch: 4 neighbours, 6 spatial
bins, radius 6, intensityThreshold = -(5 / 255) as f32.  The oracle of tests/test_gpu_liop.py; checked bit for bit against the
compiled reference through tests/golden/liop_ref.npz (tests/test_liop_model_cpu.py, tools/make_liop_fixture.py).

What is order-dependent in the reference is replayed, not re-derived:
  * patch_sort / neigh_sort are VLFeat's quicksort (vl/qsort-def.h:126-165): pivot (begin + end) / 2 swapped to the end, a Lomuto
    scan with cmp <= 0, cmp the f32 difference of two intensities (= a direct a <= b for finite floats under gradual underflow).
    The spatial bins are cut by RANK, so which of several equal pixels lies left of a bin edge is this quicksort's history;
  * a neighbour sample is (1 - wy) * (a + (b - a) * wx) + wy * (c + (d - c) * wx) in f64, in this order, rounded to f32; the bound
    tests are ix < L (not ix + 1 < L), and an operand outside the 1681 floats of the patch counts as 0.0 (the reference reads two
    floats past the patch there, times a weight of exactly 0; patch values are finite by contract);
  * threshold = -intensityThreshold * (Imax - Imin) in f32, the weight tests a > b + threshold in f64.
Everything else (the histogram of small integers, the sum of squares < 2^24) is exact in f32 in any order."""
import functools
import math

import numpy as np

L = 41
NN = 4               # neighbours
NBINS = 6            # spatial bins
RADIUS = 6.0
DIM = 24 * NBINS     # 144
THRESH = np.float32(5.0 / 255.0)     # -intensityThreshold


@functools.lru_cache(maxsize=None)
def tables():
    """(pixels [673] int64 raster indices of the measurement pixels, sx [673][4] f64, sy [673][4] f64): liop.c:346-395"""
    center = (L - 1) // 2
    t = float(np.float32(center) - np.float32(RADIUS)) + 0.6
    t2 = int(t * t)
    pixels = []
    for y in range(L):
        for x in range(L):
            if x == 0 and y == 0:
                continue
            dx, dy = x - center, y - center
            if dx * dx + dy * dy <= t2:
                pixels.append(x + y * L)
    n = len(pixels)
    sx, sy = np.zeros((n, NN)), np.zeros((n, NN))
    dangle = 2 * 3.141592653589793 / float(NN)
    for i, pixel in enumerate(pixels):
        x, y = float(pixel % L - center), float(pixel // L - center)
        angle0 = math.atan2(y, x)
        for k in range(NN):
            sx[i, k] = x + RADIUS * math.cos(angle0 + dangle * k) + center
            sy[i, k] = y + RADIUS * math.sin(angle0 + dangle * k) + center
    pixels = np.array(pixels, np.int64)
    for a in (pixels, sx, sy):
        a.setflags(write=False)
    return pixels, sx, sy


NPIX = len(tables()[0])                  # 673
BIN_AREA = NPIX // NBINS                 # 112; the last bin takes ranks 560 .. 672
EDGES = tuple(BIN_AREA * k for k in range(1, NBINS))


def vl_qsort(perm, key):
    """VL_QSORT_sort (qsort-def.h:126-197) on the index list `perm` with cmp = key[perm[i]] - key[perm[j]], in place"""
    if not perm:
        return
    stack = [(0, len(perm) - 1)]
    while stack:                          # the two recursive calls work on disjoint ranges: their order does not matter
        b, e = stack.pop()
        p = (b + e) // 2
        perm[p], perm[e] = perm[e], perm[p]
        kp = key[perm[e]]
        lp = b
        for i in range(b, e):
            if key[perm[i]] <= kp:
                perm[lp], perm[i] = perm[i], perm[lp]
                lp += 1
        perm[lp], perm[e] = perm[e], perm[lp]
        if lp > b:
            stack.append((b, lp - 1))
        if lp < e:
            stack.append((lp + 1, e))


def permutation_index(p):
    """get_permutation_index (liop.c:250-262)"""
    p = list(p)
    index = 0
    for i in range(len(p)):
        index = index * (len(p) - i) + p[i]
        for j in range(i + 1, len(p)):
            if p[j] > p[i]:
                p[j] -= 1
    return index


@functools.lru_cache(maxsize=None)
def _sample_operands():
    """per sample: the flat indices of a, b, c, d (-1 where the reference's bound test fails or the index is outside the patch)
    and wx, wy"""
    _, sx, sy = tables()
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    wx, wy = sx - ix, sy - iy
    idx = np.stack([ix + iy * L, ix + 1 + iy * L, ix + (iy + 1) * L, ix + 1 + (iy + 1) * L], -1)
    ok = np.stack([(ix >= 0) & (iy >= 0), (ix < L) & (iy >= 0), (ix >= 0) & (iy < L), (ix < L) & (iy < L)], -1)
    ok &= (idx >= 0) & (idx < L * L)
    return np.where(ok, idx, -1), wx, wy, ix, iy


def neighbour_values(patch):
    """[673][4] f32: the bilinear samples of liop.c:498-520"""
    idx, wx, wy, _, _ = _sample_operands()
    flat = np.concatenate([np.asarray(patch, np.float32).reshape(-1).astype(np.float64), [0.0]])
    a, b, c, d = (flat[idx[..., k]] for k in range(4))          # index -1: the appended 0.0
    return ((1 - wy) * (a + (b - a) * wx) + wy * (c + (d - c) * wx)).astype(np.float32)


def keys_of(patch):
    return np.asarray(patch, np.float32).reshape(-1)[tables()[0]]


def straddles(keys, perm):
    """the edges 112 k whose two sides hold equal intensities"""
    return tuple(e for e in EDGES if keys[perm[e - 1]] == keys[perm[e]])


def process(patch, perm=None):
    """vl_liopdesc_process.  perm: replaces the quicksort's permutation (the stable-sort experiments of the tests).
    -> dict(desc [144] f32, perm [673], straddle (edges), bins [673] per measurement pixel, pidx [673], weight [673], hist [144])"""
    keys = keys_of(patch)
    if perm is None:
        perm = list(range(NPIX))
        vl_qsort(perm, [float(k) for k in keys])
    perm = np.asarray(perm, np.int64)
    thr = THRESH * (keys[perm[-1]] - keys[perm[0]])               # f32 * (f32 - f32)
    assert thr.dtype == np.float32
    nv = neighbour_values(patch)
    nv64, thr64 = nv.astype(np.float64), float(thr)
    weight = np.zeros(NPIX, np.int64)
    for k in range(NN):
        for t in range(k + 1, NN):
            a, b = nv64[:, k], nv64[:, t]
            weight += (a > b + thr64) | (b > a + thr64)
    # neigh_sort per pixel.  What the quicksort does depends only on how its <= tests come out, i.e. on the order pattern of
    # the four values (each pair <, = or >): it is replayed once per pattern that occurs, on a pixel that shows it
    code = np.zeros(NPIX, np.int64)
    for k in range(NN):
        for t in range(k + 1, NN):
            code = code * 3 + (nv[:, k] > nv[:, t]).astype(np.int64) - (nv[:, k] < nv[:, t]).astype(np.int64) + 1
    pidx = np.zeros(NPIX, np.int64)
    for c, first in zip(*np.unique(code, return_index=True)):
        p = list(range(NN))
        vl_qsort(p, [float(v) for v in nv[first]])
        pidx[code == c] = permutation_index(p)
    bins = np.zeros(NPIX, np.int64)
    bins[perm] = np.minimum(np.arange(NPIX) // BIN_AREA, NBINS - 1)
    hist = np.zeros(DIM, np.int64)
    np.add.at(hist, pidx + 24 * bins, weight)
    desc = hist.astype(np.float32)                                # every partial sum of the reference is an integer < 2^24
    ssq = int((hist * hist).sum())
    assert ssq < 1 << 24
    norm = np.float32(max(math.sqrt(float(np.float32(ssq))), 1e-12))
    desc = desc / norm                                            # f32 / f32
    assert desc.dtype == np.float32
    return dict(desc=desc, perm=perm, straddle=straddles(keys, perm), bins=bins, pidx=pidx, weight=weight, hist=hist, ssq=ssq,
                nv=nv, thr=thr)


def stable_perm(patch):
    return np.argsort(keys_of(patch), kind="stable")


def describe(patches):
    """[n][144] f32 of [n][41][41] patches"""
    return np.stack([process(p)["desc"] for p in patches]) if len(patches) else np.zeros((0, DIM), np.float32)
