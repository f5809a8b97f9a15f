"""DSP-SIFT timings next to the SIFT describe calls it replaces, in one process:
    python tools/bench_dspsift.py [--reps 7]
Region sets: the regions detected on the two 1024x768 synthetic images of tools/bench_detect.py (identity view).  Per set and per
configuration (numScales 3 at 0.5 .. 1.5, numScales 15 at 0.4 .. 1.35) two things alternate `--reps` times: one
describe_regions_dspsift call, and numScales + 1 describe_regions (SIFT) calls at the same measurement sizes -- what a caller
without the entry would have to run, short of the pooling it could not do.  Both include their downloads (128 floats per region
per call).  The median wall time is reported per region, with the ratio.  The f32 norm kernel is timed alone on device rows
(sift_norm_rows_device, which returns after the kernel has finished), per call and per row.  Prints one JSON line."""
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

CONFIGS = ((3, 0.5, 1.5), (15, 0.4, 1.35))
MR = 5.1962

ctx = mods_amd.Context(0)
hip = ctypes.CDLL("libamdhip64.so")
a, b, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


out = {"sets": []}
rows_for_norm = None
for name, g in (("a", a), ("b", b)):
    im = ctx.upload(g)
    k = ctx.detect_affine_keypoints(im, mods_amd.default_hessaff_params())
    ro = ctx.detect_orientation(im, mods_amd.detect_affine_regions(k))
    regs = mods_amd.reproject_regions(ro, np.eye(3), g.shape[1], g.shape[0])
    n = len(regs)
    entry = dict(image=name, regions=n)
    for ns, c0, c1 in CONFIGS:
        sizes = [MR * (c0 + kk * (c1 - c0) / ns) for kk in range(ns + 1)]
        calls = {"dspsift": lambda: ctx.describe_regions_dspsift(im, regs, mr_size=MR, num_scales=ns, start_coef=c0, end_coef=c1),
                 "sift_calls": lambda: [ctx.describe_regions(im, regs, mr_size=mr, desc_type=0) for mr in sizes]}
        for fn in calls.values():
            fn()                                                 # warm-up: buffers
        t = {key: [] for key in calls}
        for _ in range(args.reps):
            for key, fn in calls.items():
                t[key].append(timed(fn))
        med = {key: statistics.median(v) for key, v in t.items()}
        entry["scales%d" % ns] = dict(us_per_region={key: round(1e6 * v / n, 3) for key, v in med.items()},
                                      ms_per_call={key: round(1e3 * v, 3) for key, v in med.items()},
                                      dspsift_over_sift_calls=round(med["dspsift"] / med["sift_calls"], 3))
    if rows_for_norm is None:
        rows_for_norm = ctx.describe_regions_raw(im, regs, mr_size=MR)
    out["sets"].append(entry)
    im.free()

# the norm kernel alone, on rows that stay in HBM
norm = {}
for count in (1, len(rows_for_norm), 65536):
    rows = np.ascontiguousarray(rows_for_norm[np.arange(count) % len(rows_for_norm)])
    src, dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(rows.nbytes)) == 0 and hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(rows.nbytes)) == 0
    assert hip.hipMemcpy(src, rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(rows.nbytes), 1) == 0
    ctx.sift_norm_rows_device(src.value, count, dst.value)
    ts = [timed(lambda: ctx.sift_norm_rows_device(src.value, count, dst.value)) for _ in range(max(args.reps, 21))]
    norm["rows%d" % count] = dict(us_per_call=round(1e6 * statistics.median(ts), 2), ns_per_row=round(1e9 * statistics.median(ts) / count, 2),
                                  us_min=round(1e6 * min(ts), 2))
    hip.hipFree(src)
    hip.hipFree(dst)
out["sift_norm_rows_device"] = norm
print(json.dumps(out))
ctx.close()
