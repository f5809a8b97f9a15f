"""SURF timings next to LIOP and the SIFT describe of the same regions, in one process:
    python tools/bench_surf.py [--reps 7]
Region sets: the regions detected on the two 1024x768 synthetic images of tools/bench_liop.py (identity view).  Per set the
calls -- describe_regions (RootSIFT), extract_patches into a device buffer, describe_regions_liop, describe_regions_surf --
alternate `--reps` times; the median wall time per call is reported per region together with the smallest and the largest of
the repetitions, and the ratios to the SIFT describe.  The calls include their downloads (128 / 144 / 64 floats per region).
describe_regions_surf minus extract_patches into a device buffer is what k_surf and its 64-float download add to the shared
front end.  surf_patches_device alone (rows in HBM, no front end, no copies) is timed at three sizes, per call and per patch.
Prints one JSON line."""
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
ap.add_argument("--mr-size", type=float, default=5.1962)
args = ap.parse_args()

ctx = mods_amd.Context(0)
hip = ctypes.CDLL("libamdhip64.so")
a, b, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
mr = args.mr_size


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def dev_alloc(nbytes):
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
    return p


out = {"mr_size": mr, "reps": args.reps, "sets": []}
for name, g in (("a", a), ("b", b)):
    im = ctx.upload(g)
    k = ctx.detect_affine_keypoints(im, mods_amd.default_hessaff_params())
    ro = ctx.detect_orientation(im, mods_amd.detect_affine_regions(k))
    regs = mods_amd.reproject_regions(ro, np.eye(3), g.shape[1], g.shape[0])
    n = len(regs)
    dev = dev_alloc(n * 1681 * 4)
    calls = {"sift": lambda: ctx.describe_regions(im, regs, mr_size=mr),
             "patches_device": lambda: ctx.extract_patches(im, regs, mr_size=mr, out_ptr=dev.value),
             "liop": lambda: ctx.describe_regions_liop(im, regs, mr_size=mr),
             "surf": lambda: ctx.describe_regions_surf(im, regs, mr_size=mr)}
    for fn in calls.values():
        fn()                                                     # warm-up: buffers, tables
    c0 = ctx.surf_counters()
    t = {key: [] for key in calls}
    for _ in range(args.reps):
        for key, fn in calls.items():
            t[key].append(timed(fn))
    c1 = ctx.surf_counters()
    med = {key: statistics.median(v) for key, v in t.items()}
    per = lambda v: round(1e6 * v / n, 3)      # noqa: E731
    out["sets"].append(dict(image=name, regions=n, us_per_region={key: per(v) for key, v in med.items()},
                            us_per_region_min={key: per(min(v)) for key, v in t.items()},
                            us_per_region_max={key: per(max(v)) for key, v in t.items()},
                            surf_over_sift=round(med["surf"] / med["sift"], 3), liop_over_sift=round(med["liop"] / med["sift"], 3),
                            surf_minus_patches_us_per_region=per(med["surf"] - med["patches_device"]),
                            sub_batches_per_call=(c1["sub_batches"] - c0["sub_batches"]) / args.reps))
    im.free()
    hip.hipFree(dev)

# the functor alone on rows that live in HBM
rng = np.random.default_rng(3)
out["surf_patches_device"] = []
for count in (256, 4096, 32768):
    rows = rng.uniform(0, 255, (count, 1681)).astype(np.float32)
    src, dst = dev_alloc(rows.nbytes), dev_alloc(count * 64 * 4)
    assert hip.hipMemcpy(src, rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(rows.nbytes), 1) == 0
    call = lambda: ctx.surf_patches_device(src.value, count, dst.value, mr_size=mr)      # noqa: E731
    call()
    ts = [timed(call) for _ in range(args.reps)]
    out["surf_patches_device"].append(dict(patches=count, ms=round(1e3 * statistics.median(ts), 4), ms_min=round(1e3 * min(ts), 4),
                                           ms_max=round(1e3 * max(ts), 4), us_per_patch=round(1e6 * statistics.median(ts) / count, 4)))
    hip.hipFree(src)
    hip.hipFree(dst)
print(json.dumps(out))
ctx.close()
