"""A numpy restatement of the reference's SURF descriptor functor (SURFDescriptor::operator(), descriptors/surfdescriptor.hpp:13-37
-> Integral, opensurf/integral.cpp:18-55, and Surf::getDescriptor(true), opensurf/surf.cpp:152-283) for the 41 x 41 patch that
DescribeRegions<> hands it.  The oracle of tests/test_gpu_surf.py; checked bit for bit against the compiled reference through
tests/golden/surf_ref.npz (tests/test_surf_model_cpu.py, tools/make_surf_fixture.py).

Every f32 operation is a numpy float32 operation, in the reference's order; the patches of a call are the elements of the
arrays, so each patch sees the scalar chain of the reference:
  * getGray: g = p * (float)(1.0 / 255.0) + 0.0f (OpenCV 2.4's cvConvertScale on f32, restated, not vendored);
  * Integral: a serial f32 row sum rs per row, I[r][c] = rs + I[r - 1][c];
  * one upright point at x = y = fRound(patchSize / 2.0f), scale = (float)((double)(float)patchSize / mrSize); fRound(v) =
    (int)floor(v + 0.5f) with the sum in f32;
  * BoxIntegral: indices min(., 41) - 1, zero where an index is negative, max(0.f, A - B - C + D) left to right;
  * dx, dy, mdx, mdy: serial f32 sums over the 81 samples of a sub-region in (k, l) order; len: a serial f32 sum over the 16
    sub-regions; desc[i] = (float)((double)desc[i] * (1.0 / (double)sqrtf(len))): a row of 64 NaN where len == 0;
  * the gaussian weights call the f32 exponential of the C library (the reference's object imports expf, not exp), through ctypes."""
import ctypes
import ctypes.util
import functools
import math

import numpy as np

F = np.float32
L = 41
DIM = 64
STARTS = (-12, -7, -2, 3)          # i and j of the 16 sub-regions; k in [i, i + 9), l in [j, j + 9)
NK = 24                            # distinct k (and l): -12 .. 11
PI = F(3.14159)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def expf(x):
    return F(_libm.expf(ctypes.c_float(float(F(x)))))


def fround(v):
    """fRound (opensurf/utils.h:58-61) of an f32 -> (int, whether v + 0.5f is an integer reached from a fraction of exactly .5)"""
    v = F(v)
    s = F(v + F(0.5))
    return int(math.floor(float(s))), float(v) - math.floor(float(v)) == 0.5


def gaussian_i(x, y, sig):
    """Surf::gaussian(int, int, float)"""
    return F((F(1.0) / (F(2.0) * PI * sig * sig)) * expf(F(-(x * x + y * y)) / (F(2.0) * sig * sig)))


def gaussian_f(x, y, sig):
    """Surf::gaussian(float, float, float)"""
    return F(F(1.0) / (F(2.0) * PI * sig * sig) * expf(-(x * x + y * y) / (F(2.0) * sig * sig)))


@functools.lru_cache(maxsize=None)
def tables(mr_size, patch_size=L):
    """dict(scale f32, x, y, sample_x [24], sample_y [24] (index k + 12 / l + 12), w1 [16][81] f32, w2 [16] f32, haar_size,
    ties: how many fRound calls met a fraction of exactly .5)"""
    scale = F(float(F(patch_size)) / float(mr_size))
    ties = 0
    x, t = fround(F(patch_size) / F(2.0))
    ties += t
    y = x
    co, si = F(1.0), F(0.0)
    sx, sy = np.zeros(NK, np.int64), np.zeros(NK, np.int64)
    w1, w2 = np.zeros((16, 81), F), np.zeros(16, F)
    cx = F(-0.5)
    q = 0
    for i in STARTS:
        cx = F(cx + F(1.0))
        cy = F(-0.5)
        for j in STARTS:
            cy = F(cy + F(1.0))
            ix, jx = i + 5, j + 5
            xs, t1 = fround(F(x) + (F(-jx) * scale * si + F(ix) * scale * co))
            ys, t2 = fround(F(y) + (F(jx) * scale * co + F(ix) * scale * si))
            ties += t1 + t2
            n = 0
            for k in range(i, i + 9):
                for l in range(j, j + 9):            # noqa: E741
                    sample_x, t1 = fround(F(x) + (F(-l) * scale * si + F(k) * scale * co))
                    sample_y, t2 = fround(F(y) + (F(l) * scale * co + F(k) * scale * si))
                    ties += t1 + t2
                    sx[k + 12], sy[l + 12] = sample_x, sample_y
                    w1[q, n] = gaussian_i(xs - sample_x, ys - sample_y, F(2.5) * scale)
                    n += 1
            w2[q] = gaussian_f(F(cx - F(2.0)), F(cy - F(2.0)), F(1.5))
            q += 1
    haar, t = fround(scale)
    ties += t
    for a in (sx, sy, w1, w2):
        a.setflags(write=False)
    return dict(scale=scale, x=x, y=y, sample_x=sx, sample_y=sy, w1=w1, w2=w2, haar_size=2 * haar, ties=ties)


def gray(patches):
    p = np.ascontiguousarray(patches, F).reshape(-1, L, L)
    return p * F(1.0 / 255.0) + F(0.0)


def integral(patches, columns_first=False):
    """[n][41][41] f32: Integral of getGray.  columns_first: the other order of the same sums (column prefixes, then running sums
    along the rows), for the test that shows an ordering error is visible"""
    g = gray(patches)
    n = len(g)
    out = np.zeros((n, L, L), F)
    if columns_first:
        col = np.zeros((n, L, L), F)
        for c in range(L):
            cs = np.zeros(n, F)
            for r in range(L):
                cs = cs + g[:, r, c]
                col[:, r, c] = cs
        for r in range(L):
            rs = np.zeros(n, F)
            for c in range(L):
                rs = rs + col[:, r, c]
                out[:, r, c] = rs
        return out
    for r in range(L):
        rs = np.zeros(n, F)
        for c in range(L):
            rs = rs + g[:, r, c]
            out[:, r, c] = rs + out[:, r - 1, c] if r else rs
    return out


def box_args(tab):
    """the (row, col, rows, cols) of every BoxIntegral call of a descriptor: [24 (k)][24 (l)][4 (haarX +, haarX -, haarY +, haarY -)]"""
    s = tab["haar_size"]
    h = s // 2
    out = np.zeros((NK, NK, 4, 4), np.int64)
    for a in range(NK):
        for b in range(NK):
            row, col = int(tab["sample_y"][b]), int(tab["sample_x"][a])
            out[a, b] = ((row - h, col, s, h), (row - h, col - h, s, h), (row, col - h, h, s), (row - h, col - h, h, s))
    return out


def box_integral(I, row, col, rows, cols, info=None):
    """BoxIntegral (opensurf/integral.h:35-53) on [n][41][41] integral images -> [n] f32"""
    r1, c1, r2, c2 = min(row, L) - 1, min(col, L) - 1, min(row + rows, L) - 1, min(col + cols, L) - 1
    z = np.zeros(len(I), F)
    A = I[:, r1, c1] if r1 >= 0 and c1 >= 0 else z
    B = I[:, r1, c2] if r1 >= 0 and c2 >= 0 else z
    C = I[:, r2, c1] if r2 >= 0 and c1 >= 0 else z
    D = I[:, r2, c2] if r2 >= 0 and c2 >= 0 else z
    v = A - B - C + D
    if info is not None:
        info["pre_clamp_min"] = np.minimum(info["pre_clamp_min"], v)
    return np.where(v > 0, v, F(0.0))           # std::max(0.f, v): v only where 0.f < v


def responses(I, tab, info=None):
    """(rx, ry) [n][24][24] f32: haarX / haarY at (sample_y[l], sample_x[k]), index [k + 12][l + 12]"""
    n = len(I)
    rx, ry = np.zeros((n, NK, NK), F), np.zeros((n, NK, NK), F)
    args = box_args(tab)
    for a in range(NK):
        for b in range(NK):
            bx = [box_integral(I, *(int(v) for v in args[a, b, t]), info=info) for t in range(4)]
            rx[:, a, b] = bx[0] - F(1.0) * bx[1]
            ry[:, a, b] = bx[2] - F(1.0) * bx[3]
    return rx, ry


def _chain(terms, pairwise):
    """the sum of 81 [n] f32 terms: serial from 0.f as the reference runs it, or pairwise (the ordering experiment)"""
    if not pairwise:
        acc = np.zeros_like(terms[0])
        for t in terms:
            acc = acc + t
        return acc
    level = list(terms)
    while len(level) > 1:
        level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    return level[0]


def describe(patches, mr_size, pairwise=False, columns_first=False, info=None):
    """[n][64] f32 of [n][41][41] patches.  info (optional dict): pre_clamp_min [n] (the smallest A - B - C + D of a patch), I"""
    patches = np.ascontiguousarray(patches, F).reshape(-1, L, L)
    n = len(patches)
    if n == 0:
        return np.zeros((0, DIM), F)
    tab = tables(float(mr_size))
    I = integral(patches, columns_first)            # noqa: E741
    if info is not None:
        info["pre_clamp_min"] = np.full(n, np.inf, F)
        info["I"] = I
    rx, ry = responses(I, tab, info)
    co, si = F(1.0), F(0.0)
    desc = np.zeros((n, DIM), F)
    length = np.zeros(n, F)
    q = 0
    with np.errstate(all="ignore"):
        for i in STARTS:
            for j in STARTS:
                rrx, rry = [], []
                t = 0
                for k in range(i, i + 9):
                    for l in range(j, j + 9):         # noqa: E741
                        g1 = tab["w1"][q, t]
                        x, y = rx[:, k + 12, l + 12], ry[:, k + 12, l + 12]
                        rrx.append(g1 * (-x * si + y * co))
                        rry.append(g1 * (x * co + y * si))
                        t += 1
                dx, dy = _chain(rrx, pairwise), _chain(rry, pairwise)
                mdx, mdy = _chain([np.abs(v) for v in rrx], pairwise), _chain([np.abs(v) for v in rry], pairwise)
                g2 = tab["w2"][q]
                desc[:, 4 * q + 0] = dx * g2
                desc[:, 4 * q + 1] = dy * g2
                desc[:, 4 * q + 2] = mdx * g2
                desc[:, 4 * q + 3] = mdy * g2
                length = length + (dx * dx + dy * dy + mdx * mdx + mdy * mdy) * g2 * g2
                q += 1
        length = np.sqrt(length)
        assert length.dtype == F and desc.dtype == F
        inv = 1.0 / length.astype(np.float64)
        return (desc.astype(np.float64) * inv[:, None]).astype(F)
