#!/usr/bin/env python3
"""Child process of tests/test_gpu_daisy.py:  daisy_batch_child.py IN.npz OUT.npz

MODSX_DAISY_BATCH is read once per process, so the run with sub-batches of 4 patches gets a process of its own.  It describes the
regions of IN.npz (image, regs, mr_size, params, nrm_type) with describe_regions_daisy and the patches of tests/daisy_cases.py with
daisy_patches, and writes what came back together with what each call added to Context.daisy_counters().  Nothing is compared
here."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(inp, outp):
    import mods_amd
    import daisy_cases as Cs
    z = np.load(inp)
    regs = np.frombuffer(z["regs"].tobytes(), mods_amd.REGION)
    mr = float(z["mr_size"])
    rad, radq, thq, histq = (int(v) for v in z["params"])
    nrm = int(z["nrm_type"])
    ctx = mods_amd.Context(0)
    im = ctx.upload(z["image"])
    names = mods_amd.DAISY_COUNTERS

    def delta(before):
        now = ctx.daisy_counters()
        return np.array([now[k] - before[k] for k in names], np.int64)

    c0 = ctx.daisy_counters()
    print("describe_regions_daisy", len(regs), file=sys.stderr, flush=True)
    desc = ctx.describe_regions_daisy(im, regs, mr_size=mr, rad=rad, radq=radq, thq=thq, histq=histq, nrm_type=nrm)
    d_regions = delta(c0)
    c0 = ctx.daisy_counters()
    print("daisy_patches", file=sys.stderr, flush=True)
    cases = ctx.daisy_patches(Cs.patches(), rad=rad, radq=radq, thq=thq, histq=histq, nrm_type=nrm)
    d_cases = delta(c0)
    np.savez(outp, desc=desc, cases=cases, counters_regions=d_regions, counters_cases=d_cases,
             batch=np.int64(int(os.environ.get("MODSX_DAISY_BATCH", "0"))))
    im.free()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
