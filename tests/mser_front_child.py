#!/usr/bin/env python3
"""Child process of tests/test_gpu_mser_front.py:  mser_front_child.py OUT.npz CASE [CASE ...]

MODSX_MSER_DEVICE_SORT is read once per process, so the run with the host's sort gets a process of its own.  It opens one context
and runs the named view sets of mser_front_cases.engine_cases() through run_engine() below -- the call the parent makes in its own
process with the device sort on -- and writes the region records and descriptors.  Nothing is compared here.  Progress goes to
stderr, so that the tail of a child that did not come back says where it was."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pair_params(modsx, case):
    par = modsx.default_pair_params(detector=3, ori_mrSize=5.1962)
    for k, v in case["mser"].items():
        setattr(par.mser, k, v)
    return par


def run_engine(modsx, ctx, case):
    """-> (regions, descriptors, regions per view) of one view set with the MSER detector"""
    views = modsx.set_vs_pars(case["scales"], case["tilts"], case["phi"], case["sigma"], 1, [])
    im = ctx.upload(np.ascontiguousarray(case["image"], np.float32))      # one f32 channel: stored unchanged
    try:
        return ctx.detect_describe_views(im, views, pair_params(modsx, case), want_counts=True)
    finally:
        im.free()


def main(outp, names):
    import mods_amd
    import mser_front_cases as MC
    cases = MC.engine_cases()
    ctx = mods_amd.Context(0)
    out = {}
    for name in names:
        print(name, file=sys.stderr, flush=True)
        out[name + "/regs"], out[name + "/desc"], out[name + "/counts"] = run_engine(mods_amd, ctx, cases[name])
    ctx.close()
    np.savez(outp, **out)
    print("done", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
