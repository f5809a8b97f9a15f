#!/usr/bin/env python3
"""Child process of tests/test_gpu_reps_f32.py:  reps_f32_child.py IN.npz OUT.npz

MODSX_LIOP_BATCH is read once per process, so describe_append with sub-batches of 4 patches gets a process of its own.  It
appends the regions of IN.npz (image, regs, mr_size) to the LIOP class of a fresh representation with describe_append and writes
the class's rows together with what the call added to Context.liop_counters().  Nothing is compared here."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(inp, outp):
    import mods_amd
    z = np.load(inp)
    regs = np.frombuffer(z["regs"].tobytes(), mods_amd.REGION)
    ctx = mods_amd.Context(0)
    im = ctx.upload(z["image"])
    rep = mods_amd.Rep(ctx)
    c0 = ctx.liop_counters()
    print("describe_append", len(regs), file=sys.stderr, flush=True)
    n = rep.describe_append(im, regs, 0, mods_amd.DESC_LIOP, mr_size=float(z["mr_size"]))
    c1 = ctx.liop_counters()
    got_regs, rows = rep.class_f32(0, mods_amd.DESC_LIOP)
    np.savez(outp, n=np.int64(n), rows=rows, ids=got_regs["id"], counters=np.array([c1[k] - c0[k] for k in mods_amd.LIOP_COUNTERS], np.int64),
             batch=np.int64(int(os.environ.get("MODSX_LIOP_BATCH", "0"))))
    rep.free()
    im.free()
    ctx.close()


if __name__ == "__main__":
    main(*sys.argv[1:3])
