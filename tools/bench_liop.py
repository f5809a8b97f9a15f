"""LIOP and patch-out timings next to the SIFT describe of the same regions, in one process:
    python tools/bench_liop.py [--reps 7]
Region sets: the regions detected on the two 1024x768 synthetic images of tools/bench_detect.py (identity view).  Per set the
three calls -- describe_regions (RootSIFT), extract_patches, describe_regions_liop -- alternate `--reps` times and the median
wall time per call is reported per region, with the ratios to the SIFT describe.  The calls include their downloads (128 / 1681 /
144 floats per region), so extract_patches is also timed into a device buffer.  The exact-path share comes from the counters.
The disc-constant patch -- every measurement pixel equal, the quicksort's worst case -- is timed alone and in a batch through
liop_patches.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mods_amd  # noqa: E402
from mods_amd import synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

ctx = mods_amd.Context(0)
hip = ctypes.CDLL("libamdhip64.so")
a, b, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


out = {"sets": []}
for name, g in (("a", a), ("b", b)):
    im = ctx.upload(g)
    k = ctx.detect_affine_keypoints(im, mods_amd.default_hessaff_params())
    ro = ctx.detect_orientation(im, mods_amd.detect_affine_regions(k))
    regs = mods_amd.reproject_regions(ro, np.eye(3), g.shape[1], g.shape[0])
    n = len(regs)
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), ctypes.c_size_t(n * 1681 * 4)) == 0
    calls = {"sift": lambda: ctx.describe_regions(im, regs), "patches": lambda: ctx.extract_patches(im, regs),
             "patches_device": lambda: ctx.extract_patches(im, regs, out_ptr=dev.value),
             "liop": lambda: ctx.describe_regions_liop(im, regs)}
    for fn in calls.values():
        fn()                                                     # warm-up: buffers, tables
    c0 = ctx.liop_counters()
    t = {key: [] for key in calls}
    for _ in range(args.reps):
        for key, fn in calls.items():
            t[key].append(timed(fn))
    c1 = ctx.liop_counters()
    med = {key: statistics.median(v) for key, v in t.items()}
    out["sets"].append(dict(image=name, regions=n, us_per_region={key: round(1e6 * v / n, 3) for key, v in med.items()},
                            liop_over_sift=round(med["liop"] / med["sift"], 3), patches_over_sift=round(med["patches"] / med["sift"], 3),
                            patches_device_over_sift=round(med["patches_device"] / med["sift"], 3),
                            exact_path_share=(c1["exact_path"] - c0["exact_path"]) / max(1, c1["regions"] - c0["regions"]),
                            sub_batches_per_call=(c1["sub_batches"] - c0["sub_batches"]) / args.reps))
    im.free()
    hip.hipFree(dev)

# the worst case alone, and 256 of it at once
pix = mods_amd.liop_tables()[0]
worst = np.random.default_rng(1).uniform(0, 255, (41, 41)).astype(np.float32)
worst.reshape(-1)[pix] = np.float32(128.0)
easy = np.random.default_rng(2).uniform(0, 255, (41, 41)).astype(np.float32)
for label, p in (("disc_constant", worst), ("distinct", easy)):
    for count in (1, 256):
        rows = np.repeat(p[None], count, 0)
        ctx.liop_patches(rows)
        out["%s_x%d_ms" % (label, count)] = round(1e3 * statistics.median(timed(lambda: ctx.liop_patches(rows)) for _ in range(args.reps)), 4)
print(json.dumps(out))
ctx.close()
