#!/usr/bin/env python3
"""Child process of tests/test_gpu_views_shared_rotation.py:  views_share_child.py IN.npz OUT.npz

MODSX_VIEWS_SHARE_ROT is read once per process, so the switched-off run gets a process of its own.  It opens one context and
synthesises the headline ladder of IN's image as one launch set -- the call the parent makes in its own process with the sharing
on -- and writes the views and the view counters.  Nothing is compared here.  Progress goes to stderr, so that the tail of a child
that did not come back says where it was."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADLINE = ([1.0], [1, 2, 4, 6, 8], 120.0, 0.2, 1)     # the 31 views bench.py measures


def run_ladder(modsx, ctx, image, log=lambda s: None):
    """-> dict of arrays: view_%02d per non-identity view, counters = (views fused, groups, rotated pixels) of the one call"""
    views = modsx.set_vs_pars(*HEADLINE, [])
    log("upload")
    im = ctx.upload(np.ascontiguousarray(image, np.float32))
    modsx.views_counters(reset=True)
    log("synth")
    got = ctx.synth_views([im] * len(views), views)
    out = {"counters": np.array(modsx.views_counters(reset=True), np.int64)}
    log("download")
    for i, (g, ident) in enumerate(got):
        if not ident:
            out["view_%02d" % i] = g.download()
        g.free()
    im.free()
    return out


def main(inp, outp):
    import mods_amd
    z = np.load(inp)
    ctx = mods_amd.Context(0)
    out = run_ladder(mods_amd, ctx, z["image"], log=lambda s: print(s, file=sys.stderr, flush=True))
    ctx.close()
    np.savez(outp, **out)
    print("done", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
