#!/usr/bin/env python3
"""Child process of tests/test_gpu_surf.py:  surf_batch_child.py IN.npz OUT.npz

MODSX_SURF_BATCH is read once per process, so the run with sub-batches of 4 patches gets a process of its own.  It describes the
regions of IN.npz (image, regs, mr_size) with describe_regions_surf and the patches of tests/surf_cases.py with surf_patches, and
writes what came back together with what each call added to Context.surf_counters().  Nothing is compared here."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(inp, outp):
    import mods_amd
    import surf_cases as Cs
    z = np.load(inp)
    regs = np.frombuffer(z["regs"].tobytes(), mods_amd.REGION)
    mr = float(z["mr_size"])
    ctx = mods_amd.Context(0)
    im = ctx.upload(z["image"])
    names = mods_amd.SURF_COUNTERS

    def delta(before):
        now = ctx.surf_counters()
        return np.array([now[k] - before[k] for k in names], np.int64)

    c0 = ctx.surf_counters()
    print("describe_regions_surf", len(regs), file=sys.stderr, flush=True)
    desc = ctx.describe_regions_surf(im, regs, mr_size=mr)
    d_regions = delta(c0)
    c0 = ctx.surf_counters()
    print("surf_patches", file=sys.stderr, flush=True)
    cases = ctx.surf_patches(Cs.patches(), mr_size=mr)
    d_cases = delta(c0)
    np.savez(outp, desc=desc, cases=cases, counters_regions=d_regions, counters_cases=d_cases,
             batch=np.int64(int(os.environ.get("MODSX_SURF_BATCH", "0"))))
    im.free()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
