#!/usr/bin/env python3
"""Child process of tests/test_gpu_describe_chunks.py:  describe_chunk_child.py IN.npz OUT.npz

MODSX_ARENA_MB is read once per process, so the run with the 16 MiB window arena gets a process of its own.  It opens one context
and makes the calls of run_all() below -- the ones the parent makes in its own process at the default arena -- and writes what they
returned together with what every call added to Context.describe_counters() and, for the views and the crafted case, with what
the planner alone (mods_amd.describe_plan, no device) gives for the same regions at this process's arena.  Nothing is compared
here.  Progress goes to stderr, so that the tail of a child that did not come back says where it was."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import describe_cases as DC     # noqa: E402

PAIR_SCALARS = ("n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples", "ransac_lo")
RANSAC_SEED = 9
TWO_CLASSES = ((1, 0.8), (3, 0.8))       # the WxBS descriptor list: RootSIFT + HalfRootSIFT


def views_of(modsx):
    return modsx.set_vs_pars([1.0], list(DC.VIEW_TILTS), 360.0, 0.5, 1, [])


def _delta(modsx, ctx, before):
    now = ctx.describe_counters()
    d = {k: now[k] - before[k] for k in modsx.DESCRIBE_COUNTERS}
    d["max_chunks"] = now["max_chunks"]          # a running maximum, not a sum: the parent reads it per case in call order
    return np.array([d[k] for k in modsx.DESCRIBE_COUNTERS], np.int64)


def _plan(modsx, lists, mr_size):
    p = modsx.describe_plan(lists, mr_size, arena_floats=DC.arena_floats())
    assert p["rc"] == 0, p
    return np.array([p["counters"][k] for k in modsx.DESCRIBE_COUNTERS], np.int64)


def run_all(modsx, ctx, small_a, small_b, log=lambda s: None):
    """-> dict of arrays: the three chunk cases, each with what it added to the describe counters (max_chunks: the reading
    after the case); views_plan / crafted_plan: the planner's counters of the same regions (the views as 11 images)"""
    out = {}
    log("views")
    im = ctx.upload(np.ascontiguousarray(small_a, np.float32))
    c0 = ctx.describe_counters()
    regs, desc, counts = ctx.detect_describe_views(im, views_of(modsx), modsx.default_pair_params(desc_mrSize=DC.VIEWS_DESC_MR),
                                                   want_counts=True)
    out["views_counters"] = _delta(modsx, ctx, c0)
    out["views_regs"], out["views_desc"], out["views_per_view"] = regs, desc, counts
    # the 11 views go through one describe_batch call, view by view in list order: its images are the views' region lists
    out["views_plan"] = _plan(modsx, np.split(regs, np.cumsum(counts)[:-1]), DC.VIEWS_DESC_MR)
    im.free()
    log("crafted")
    im = ctx.upload(DC.image())
    c0 = ctx.describe_counters()
    out["crafted_desc"] = ctx.describe_regions(im, DC.crafted_regions().view(modsx.REGION), mr_size=DC.MR_SIZE)
    out["crafted_counters"] = _delta(modsx, ctx, c0)
    out["crafted_plan"] = _plan(modsx, DC.crafted_regions(), DC.MR_SIZE)
    im.free()
    log("pair")
    ia, ib = ctx.upload(small_a), ctx.upload(small_b)
    c0 = ctx.describe_counters()
    r = ctx.match_pair(ia, ib, modsx.default_pair_params(ransac_seed=RANSAC_SEED, desc_mrSize=DC.VIEWS_DESC_MR, descs=list(TWO_CLASSES)))
    out["pair_counters"] = _delta(modsx, ctx, c0)
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
    out = run_all(mods_amd, ctx, z["small_a"], z["small_b"], log=lambda s: print(s, file=sys.stderr, flush=True))
    ctx.close()
    np.savez(outp, **out)
    print("done", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
