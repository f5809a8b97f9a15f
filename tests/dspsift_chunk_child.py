#!/usr/bin/env python3
"""Child process of tests/test_gpu_dspsift.py:  dspsift_chunk_child.py OUT.npz

MODSX_ARENA_MB is read once per process, so the run whose scale passes are cut into chunks gets a process of its own.  It
describes dspsift_cases.chunk_regions() on describe_cases.image() with describe_regions_dspsift at CHUNK_CONFIG and writes what
came back with what the call added to Context.describe_counters() and Context.dsp_counters().  Nothing is compared here."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(ctx, modsx):
    """-> dict(desc, describe_counters, dsp_counters) of the one call, on the caller's context"""
    import dspsift_cases as Cs
    from tests import describe_cases as DC
    ns, a, b = Cs.CHUNK_CONFIG
    im = ctx.upload(DC.image())
    try:
        c0, d0 = ctx.describe_counters(), ctx.dsp_counters()
        desc = ctx.describe_regions_dspsift(im, Cs.chunk_regions(), mr_size=DC.MR_SIZE, num_scales=ns, start_coef=a, end_coef=b)
        c1, d1 = ctx.describe_counters(), ctx.dsp_counters()
    finally:
        im.free()
    return dict(desc=desc,
                describe_counters=np.array([c1[k] - c0[k] for k in modsx.DESCRIBE_COUNTERS], np.int64),
                dsp_counters=np.array([d1[k] - d0[k] for k in modsx.DSP_COUNTERS], np.int64))


def main(outp):
    import mods_amd
    ctx = mods_amd.Context(0)
    print("describe_regions_dspsift at MODSX_ARENA_MB=%s" % os.environ.get("MODSX_ARENA_MB"), file=sys.stderr, flush=True)
    out = run(ctx, mods_amd)
    np.savez(outp, arena_mb=np.int64(int(os.environ.get("MODSX_ARENA_MB", "0"))), **out)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1])
