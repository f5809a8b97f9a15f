#!/usr/bin/env python3
"""Child process of tests/test_gpu_orient_prefilter.py:  orient_prefilter_child.py IN.npz OUT.npz

MODSX_ORI_PREFILTER is read once per process, so the switched-off run gets a process of its own.  It opens one context and makes
the calls of run_all() below -- the ones the parent makes in its own process with the filter on -- and writes what they returned
together with the orientation counters.  Nothing is compared here.  Progress goes to stderr, so that the tail of a child that
did not come back says where it was."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS = ((1.0, 0.0), (2.0, np.pi / 3), (4.0, np.pi / 6))     # (tilt, phi): identity, tilt 2 at 60 degrees, tilt 4 at 30 degrees
PAIR_SCALARS = ("n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples", "ransac_lo")
RANSAC_SEED = 9


def run_all(modsx, ctx, image_u8, small_a, small_b, log=lambda s: None):
    """-> dict of arrays: the three views of image_u8 through the views API and small_a / small_b through match_pairs (the
    single-view batch path), each with the (launched, skipped) it added to the orientation counters"""
    out = {}
    views = [modsx.make_view(t, p) for t, p in VIEWS]
    log("views")
    im = ctx.upload(np.ascontiguousarray(image_u8, np.uint8))          # u8 in, f32 on the device
    modsx.orientation_counts(reset=True)
    regs, desc, counts = ctx.detect_describe_views(im, views, modsx.default_pair_params(), want_counts=True)
    out["views_counts"] = np.array(modsx.orientation_counts(reset=True), np.int64)
    out["views_regs"], out["views_desc"], out["views_per_view"] = regs, desc, counts
    im.free()
    log("pair")
    ia, ib = ctx.upload(small_a), ctx.upload(small_b)
    r = modsx.match_pairs([ctx], [ia], [ib], modsx.default_pair_params(ransac_seed=RANSAC_SEED))[0]
    out["pair_counts"] = np.array(modsx.orientation_counts(reset=True), np.int64)
    out["pair_regions"] = np.array(r["n_regions"])
    out["pair_scalars"] = np.array([r[f] for f in PAIR_SCALARS])
    out["pair_tentatives"] = r["tentatives"]
    out["pair_ransac_inlier"] = np.asarray(r["ransac_inlier"])
    out["pair_verified"] = np.asarray(r["verified"])
    out["pair_H"] = np.asarray(r["H"])
    ia.free(); ib.free()
    return out


def main(inp, outp):
    import mods_amd
    z = np.load(inp)
    ctx = mods_amd.Context(0)
    out = run_all(mods_amd, ctx, z["image_u8"], z["small_a"], z["small_b"], log=lambda s: print(s, file=sys.stderr, flush=True))
    ctx.close()
    np.savez(outp, **out)
    print("done", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
