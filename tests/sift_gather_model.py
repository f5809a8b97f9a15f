"""k_describe's choice between its two histogram gathers (mods_amd/csrc/kernels_describe.hip, "samplePatch, order-free form"), restated
in numpy for ONE region, statement by statement: what is a float in the kernel is np.float32 here, the bin sums are 64-bit integers.

  stages(patch)    the per-pixel stage in front of the gather: gradients, |grad|, the atan2 table entry (code, idx, special), the
                   fractional orientation bin o of the kernel's oTab, val = mask * |grad|
  decide(patch)    mxb, E, scalable, S; the eight scaled terms of every pixel; tmin; the integer bin sums X; the three triggers
                   of the ordered gather and `inexact`; and the order-free result ldexp(X, E - 47)
  photo_norm(p)    photometricallyNormalize as the kernel runs it (f32 running sums over the masked pixels in raster order), used
                   by the case module's searches; tests/test_sift_patch_cases_cpu.py ties it to the oracle

`patch` is what the gather sees: the planted patch under photo_norm = 0, the normalised one under photo_norm = 1.  The reference of
the histogram itself is tests/dspsift_model.py (histogram_f64: the terms added in the reference's order); this module only says
which gather the kernel takes and what the order-free one returns.

What the arithmetic allows (proved here, established on the cases by the CPU test; see also sift_patch_cases.E_REACHABLE):
  * a finite |grad| is below 2^64 (the f32 sum xg^2 + yg^2 is finite), the mask is at most 1: E <= 64 whenever `scalable` can hold;
  * a nonzero |grad| is at least 2^-74.5 (the smallest f32 above zero is 2^-149) and a nonzero mask at least exp(-1 / 0.9): a
    nonzero val is above 2^-77, so E >= -76;
  * with S = 2^(47 - E) >= 2^-17 a positive val scales to at least 2^-94, and its smallest term -- times row and column weights of
    at least 1/8 and an orientation weight of at least 2^-21 (o is an f32 in [4, 16)) -- to at least 2^-121: no positive val
    scales to zero or to a subnormal, every term below 2^23 is seen by tmin;
  * a bin adds at most one term per pixel of its 16 x 16 block, the row and the column weights of a block sum to 8 each and the
    orientation weight is at most 1: X <= 64 * max scaled val < 64 * 2^47 = 2^53.  The third trigger (a bin at 2^53 or more) can
    NOT be reached; BIN_BOUND below is that bound and the CPU test checks it on every case.
"""
import numpy as np

import dspsift_model as D
import orient_model as OM

f32, f64 = np.float32, np.float64
PS, NPX = D.PS, D.NPX
E_MIN, E_MAX = -60, 64                  # `scalable` of the kernel: E >= -60 && E <= 64
BIN_BOUND = 64 * (1 << 47)              # = 2^53: strictly above every X
TRIGGERS = ("not_scalable", "small_term", "big_bin")

_lut = None


def lut():
    global _lut
    if _lut is None:
        from oracle import pyoracle as O
        _lut = np.asarray(O.atan_lut(), f64)
    return _lut


def o_table():
    """the kernel's oTab (engine.hip, upload_tables): [8 * 256 + 1] f32, o = (float)(8 * (ori + 2 pi) / (2 pi)); entry 2048 = the special case"""
    e = np.arange(2048)
    ori = np.concatenate([OM.angle_of_case(lut(), e >> 8, e & 255), np.zeros(1, f32)]).astype(f32)
    return ((f64(f32(8.0)) * (ori.astype(f64) + D.TWO_PI)) / D.TWO_PI).astype(f32)


def stages(patch):
    p = np.ascontiguousarray(patch, f32).reshape(PS, PS)
    xg, yg = np.empty((PS, PS), f32), np.empty((PS, PS), f32)
    with np.errstate(all="ignore"):
        xg[:, 1:-1] = p[:, 2:] - p[:, :-2]
        xg[:, 0] = p[:, 1] - p[:, 0]
        xg[:, -1] = p[:, -1] - p[:, -2]
        yg[1:-1] = p[2:] - p[:-2]
        yg[0] = p[1] - p[0]
        yg[-1] = p[-1] - p[-2]
        g = np.sqrt(xg * xg + yg * yg)
        code, idx, special = OM.atan_case(yg, xg)
        entry = np.where(special, 2048, code * 256 + idx)
        vv = D.mask() * g
    return dict(xg=xg, yg=yg, g=g, code=code, idx=idx, special=special, entry=entry, o=o_table()[entry], vv=vv.astype(f32))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def decide(patch):
    st = stages(patch)
    vv, o = st["vv"].reshape(-1), st["o"].reshape(-1)
    mxb = int((_bits(vv) & np.uint32(0x7fffffff)).max())
    E = (mxb >> 23) - 126
    scalable = 0x00800000 <= mxb < 0x7f800000 and E_MIN <= E <= E_MAX
    Es = E if scalable else 47
    S = f32(2.0 ** (47 - Es))
    b0, b1, w0, w1 = D.bins_and_weights()
    w0, w1 = w0.astype(f32), w1.astype(f32)
    wm = np.where(w0 > 0, np.where(w1 > 0, np.minimum(w0, w1), w0), np.where(w1 > 0, w1, f32(1)))
    r, c = (a.reshape(-1) for a in np.mgrid[0:PS, 0:PS])
    with np.errstate(all="ignore"):
        val = vv * S
        live = val > 0
        bo0 = np.where(live, o, f32(8)).astype(np.int64)
        wo1 = o - bo0.astype(f32)
        wo0 = f32(1.0) - wo1
        wc0, wc1 = w0[c] * val, w1[c] * val
        # bins_and_weights' bins are already x 8: bin = 32 rb + 8 cb + slot = 4 b[r] + b[c] + slot
        quads = ((wc0 * w0[r], 4 * b0[r] + b0[c]), (wc1 * w0[r], 4 * b0[r] + b1[c]),
                 (wc0 * w1[r], 4 * b1[r] + b0[c]), (wc1 * w1[r], 4 * b1[r] + b1[c]))
        X = np.zeros(128, np.uint64)
        nterms = 0
        for v, cell8 in quads:
            for wo, slot in ((wo0, bo0 & 7), (wo1, (bo0 + 1) & 7)):
                t = (wo * v).astype(f64)
                ok = live & np.isfinite(t) & (t < 2.0 ** 52)
                # (double)t + 2^52 holds round-to-nearest-even(t) in its low 52 bits
                np.add.at(X, cell8 + slot, np.rint(np.where(ok, t, 0.0)).astype(np.uint64))
                nterms += int((ok & (t > 0)).sum())
        wom = np.where(wo1 > 0, np.minimum(wo0, wo1), wo0)
        small = ((wm[r] * (wm[c] * val)) * wom).astype(f32)
        tb = (_bits(small).astype(np.int64) - 1) & 0xffffffff
        m = int(tb[live].min()) if live.any() else 0xffffffff
    trig = dict(not_scalable=not scalable, small_term=m != 0xffffffff and ((m + 1) & 0xffffffff) < 0x4b000000,
                big_bin=bool((X >> np.uint64(53)).any()))
    return dict(mxb=mxb, E=E, scalable=scalable, S=S, X=X, tmin=m, triggers=trig, inexact=any(trig.values()),
                order_free=np.ldexp(X.astype(f64), Es - 47), live=int(live.sum()), nterms=nterms,
                val_min=float(vv[vv > 0].min()) if (vv > 0).any() else 0.0, stages=st)


def photo_stats(patch):
    """(mean, var) of photometricallyNormalize: f32 running sums over the masked pixels in raster order (np.cumsum adds in order)"""
    p = np.ascontiguousarray(patch, f32).reshape(-1)
    v = p[D.mask().reshape(-1) > 0]
    n = f32(len(v))
    with np.errstate(all="ignore"):
        mean = np.cumsum(v, dtype=f32)[-1] / n
        d = mean - v
        var = np.sqrt(np.cumsum(d * d, dtype=f32)[-1] / n)
    return f32(mean), f32(var)


def photo_norm(patch):
    p = np.ascontiguousarray(patch, f32).reshape(PS, PS)
    mean, var = photo_stats(p)
    if f64(var) < 0.0001:
        return p.copy()
    with np.errstate(all="ignore"):
        fac = f32(50.0) / var
        v = f32(128.0) + fac * (p - mean)
        v = np.where(v > f32(255), f32(255), v)          # a NaN fails both comparisons and stays, as in the kernel
        v = np.where(v < f32(0), f32(0), v)
    return v.astype(f32)
