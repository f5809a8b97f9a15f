"""Inputs and CPU references of tests/test_gpu_describe_slim.py, and the child of its MODSX_DESCRIBE_SLIM=0 case (run as a
script: `python describe_slim_cases.py OUT.npz` describes every list of `lists()` and stores the descriptors).  No GPU in the
module itself.

One 256 x 256 image: columns 64 .. 191 hold smooth noise, the 64 columns on either side are zeros.  Regions have A = I and
s = 1 and are described with mr_size = 10 and fast = 0: ceil(s * mr_size) = 10 > 8.2, a 21-pixel measurement window
(imageToPatchScale 21 / 41 > 0.4), i.e. the grid branch with P = 23.  A region centred in a blank strip sees zeros only (the blur of
zeros is zeros), is not scalable and forces the ordered gather on its workgroup (sift_patch_cases: the FORCER).  A region with
s = 0.3 has a 7-pixel window (7 / 41 <= 0.4): the direct branch.
"""
import os
import sys

import numpy as np

import dspsift_model as D
import sift_gather_model as G
import sift_patch_cases as SC

F = np.float32
MR_SIZE, FAST = 10.0, 0
SIZE, LEFT, RIGHT = 256, 64, 192
TEX = [(100, 32), (150, 32), (100, 96), (150, 96), (125, 160), (90, 160)]      # textured centres (x, y), two per 64-row band
ZERO_L = [(30, 32), (30, 96)]                                                  # blank centres left of the texture ...
ZERO_R = [(225, 32), (225, 96)]                                                # ... and right of it
SMALL_S = 0.3
TWO_CLASSES = ((1, 0.8), (3, 0.8))          # RootSIFT + HalfRootSIFT in one step
PAIR_DESC_MR = 24.0                         # every region of the pair case takes the grid branch

_image = None
_ref = {}


def image():
    global _image
    if _image is None:
        import orient_cases as OC
        rs = np.random.RandomState(2601)
        img = np.zeros((SIZE, SIZE), F)
        img[:, LEFT:RIGHT] = (OC._smooth(rs.standard_normal((SIZE, RIGHT - LEFT)).astype(F) * F(60), 2) + F(100))
        img.setflags(write=False)
        _image = img
    return _image


def regions(dtype, centres, s=1.0):
    return SC.regions(dtype, centres, s)


def zero_centres(n):
    """n centres inside the two blank strips, all of them 12 pixels or more from the texture and the border"""
    xs = list(range(14, 51, 6)) + list(range(206, 243, 6))
    ys = list(range(14, 243, 12))
    out = [(x, y) for y in ys for x in xs]
    assert len(out) >= n
    return out[:n]


def lists():
    """name -> (centres, scales): every region list the GPU test describes (the child describes the same)"""
    big = zero_centres(140)
    return {
        "free_even": (TEX[:4], None),
        "free_odd": (TEX[:3], None),
        "forced_slot1": ([TEX[0], ZERO_R[0], TEX[2], TEX[3]], None),           # band 0: (textured, zero); band 1: order-free
        "forced_slot0": ([ZERO_L[0], TEX[0], ZERO_L[1], TEX[2]], None),        # (zero, textured) twice
        "long_redo": (big[:70] + [TEX[0], TEX[5]] + big[70:], None),           # 140 zero regions + 2 textured: > 64 redo workgroups
        "mixed_direct": (TEX[:4] + [TEX[4]], [1.0] * 4 + [SMALL_S]),
    }


def reference(oracle, modsx, centre, photo_norm):
    """dict(patch: the oracle's normalised patch of the region, decision: sift_gather_model.decide on it, desc {type: [128]})"""
    key = (tuple(centre), photo_norm)
    if key not in _ref:
        reg = regions(modsx.REGION, [centre])
        raw = oracle.extract_patch(image(), reg[0], mr_size=MR_SIZE)
        d1, npatch = oracle.describe_patch(raw, photo_norm=photo_norm, rootsift=1)
        d0, _ = oracle.describe_patch(raw, photo_norm=photo_norm, rootsift=0)
        npatch = npatch.reshape(SC.PS, SC.PS)
        with np.errstate(all="ignore"):
            hist = D.histogram_f64(npatch)
            half = {dt: D.describe_f64(hist, dt) for dt in (2, 3)}
        _ref[key] = dict(patch=npatch, decision=G.decide(npatch), desc={0: d0, 1: d1, 2: half[2], 3: half[3]},
                         raw=hist.astype(F))
    return _ref[key]


def inexact(oracle, modsx, centres, photo_norm):
    return np.array([reference(oracle, modsx, c, photo_norm)["decision"]["inexact"] for c in centres])


def describe_all(modsx, ctx, handle):
    """every list of lists() under photo_norm 1 and RootSIFT -> dict name -> [n, 128]"""
    out = {}
    for name, (cen, scales) in lists().items():
        regs = regions(modsx.REGION, cen) if scales is None else np.concatenate(
            [regions(modsx.REGION, [c], s) for c, s in zip(cen, scales)])
        out[name] = ctx.describe_regions(handle, regs, mr_size=MR_SIZE, fast=FAST, photo_norm=1, desc_type=1)
    return out


def pair_result(modsx, ctx, small_pair):
    """match_pair of the suite's small synthetic pair with two descriptor classes in one step -> dict of arrays"""
    a, b, _ = small_pair
    ia, ib = ctx.upload(a), ctx.upload(b)
    try:
        r = ctx.match_pair(ia, ib, modsx.default_pair_params(ransac_seed=9, desc_mrSize=PAIR_DESC_MR, descs=list(TWO_CLASSES)))
    finally:
        ia.free(); ib.free()
    t = r["tentatives"]
    out = {"pair_n_regions": np.array(r["n_regions"]), "pair_n_unique": np.array(r["n_unique"]),
           "pair_ransac_inlier": np.asarray(r["ransac_inlier"])}
    for f in t.dtype.names:
        out["pair_t_" + f] = np.ascontiguousarray(t[f])
    return out


def main(outp):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import mods_amd
    from mods_amd import synthetic
    ctx = mods_amd.Context(0)
    handle = ctx.upload(image())
    out = describe_all(mods_amd, ctx, handle)
    handle.free()
    out.update(pair_result(mods_amd, ctx, synthetic.make_pair(rows=240, cols=320, nblobs=420, seed=777)))
    c = ctx.describe_slim_counters()
    out["slim_counters"] = np.array([c[k] for k in mods_amd.DESCRIBE_SLIM_COUNTERS], np.int64)
    ctx.close()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1])
