#!/usr/bin/env python3
"""Child process of tests/test_gpu_{liop,surf,daisy}.py:  patchdesc_batch_child.py {liop,surf,daisy} IN.npz OUT.npz

MODSX_<NAME>_BATCH is read once per process, so the run with sub-batches of 4 patches gets a process of its own.  It describes the
regions of IN.npz (image, regs, mr_size; for daisy also params, nrm_type) with describe_regions_<name> and the patches of
tests/<name>_cases.py with <name>_patches, and writes what came back together with what each call added to
Context.<name>_counters().  Nothing is compared here."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(name, inp, outp):
    import mods_amd
    Cs = importlib.import_module(name + "_cases")
    z = np.load(inp)
    regs = np.frombuffer(z["regs"].tobytes(), mods_amd.REGION)
    mr = float(z["mr_size"])
    # what the descriptor takes besides the rows: (of describe_regions_<name>, of <name>_patches)
    if name == "liop":
        kw_regions, kw_patches = dict(mr_size=mr), {}
    elif name == "surf":
        kw_regions = kw_patches = dict(mr_size=mr)
    else:
        rad, radq, thq, histq = (int(v) for v in z["params"])
        kw_patches = dict(rad=rad, radq=radq, thq=thq, histq=histq, nrm_type=int(z["nrm_type"]))
        kw_regions = dict(kw_patches, mr_size=mr)
    ctx = mods_amd.Context(0)
    im = ctx.upload(z["image"])
    names = getattr(mods_amd, name.upper() + "_COUNTERS")
    counters = getattr(ctx, name + "_counters")

    def delta(before):
        now = counters()
        return np.array([now[k] - before[k] for k in names], np.int64)

    c0 = counters()
    print("describe_regions_" + name, len(regs), file=sys.stderr, flush=True)
    desc = getattr(ctx, "describe_regions_" + name)(im, regs, **kw_regions)
    d_regions = delta(c0)
    c0 = counters()
    print(name + "_patches", file=sys.stderr, flush=True)
    cases = getattr(ctx, name + "_patches")(Cs.patches(), **kw_patches)
    d_cases = delta(c0)
    np.savez(outp, desc=desc, cases=cases, counters_regions=d_regions, counters_cases=d_cases,
             batch=np.int64(int(os.environ.get("MODSX_%s_BATCH" % name.upper(), "0"))))
    im.free()
    ctx.close()


if __name__ == "__main__":
    main(*sys.argv[1:4])
