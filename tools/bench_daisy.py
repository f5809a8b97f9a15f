"""DAISY timings next to SURF and the SIFT describe of the same regions, in one process:
    python tools/bench_daisy.py [--reps 7]
Region sets: the regions detected on the two 1024x768 synthetic images of tools/bench_surf.py (identity view).  Per set the calls
-- describe_regions (RootSIFT), extract_patches into a device buffer, describe_regions_surf, describe_regions_daisy at the
reference's defaults (rad 15) and at the shipped ini's rad 20 -- alternate `--reps` times; the median wall time per call is
reported per region together with the smallest and the largest of the repetitions, and the ratios to the SIFT describe.  The
calls include their downloads (128 / 64 / 200 floats per region).  daisy_patches_device alone (rows in HBM, no front end, no
copies) is timed at both parameter sets, per call and per patch, next to bounds computed from the kernel's tap counts
(kernels_daisy.hip: a filter pass of a plane is 246 work items that each run 7 chains of ksize unfused multiply-adds and read
their window in blocks of 8 samples, ceil((ksize + 6) / 8) blocks, every sample of a block feeding all 7 chains; 8 layers, 2
passes per filter):
  lds_bound_us_per_patch     the words read and written in the filter passes at 128 B per clock and CU (ds_read_b32);
  valu_bound_us_per_patch    two VALU operations per tap and output -- what the arithmetic needs -- at 64 lanes per clock and CU;
  valu_issued_us_per_patch   the same for the multiply-adds the kernel issues, zero taps of the padded blocks included;
all for 256 CUs at 2.4 GHz with every CU busy.  Prints one JSON line."""
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

CUS, HZ = 256, 2.4e9
PARAMS = {"default": dict(rad=15, radq=3, thq=8, histq=8), "ini": dict(rad=20, radq=3, thq=8, histq=8)}

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


def bounds(p):
    fsz = [int(v) for v in mods_amd.daisy_tables(**p)["fsz"]]
    items = 8 * 2 * 246
    steps = [8 * ((k + 6 + 7) // 8) for k in fsz]
    lds_words = items * sum(steps) + 8 * 2 * 1681 * len(fsz)
    valu_ops, valu_issued = items * 7 * sum(fsz) * 2, items * 7 * sum(steps) * 2
    return dict(taps=fsz, lds_bound_us_per_patch=round(1e6 * lds_words * 4 / (128 * CUS * HZ), 4),
                valu_bound_us_per_patch=round(1e6 * valu_ops / (64 * CUS * HZ), 4),
                valu_issued_us_per_patch=round(1e6 * valu_issued / (64 * CUS * HZ), 4))


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
             "surf": lambda: ctx.describe_regions_surf(im, regs, mr_size=mr),
             "daisy_default": lambda: ctx.describe_regions_daisy(im, regs, mr_size=mr, **PARAMS["default"]),
             "daisy_ini": lambda: ctx.describe_regions_daisy(im, regs, mr_size=mr, **PARAMS["ini"])}
    for fn in calls.values():
        fn()                                                     # warm-up: buffers, tables
    c0 = ctx.daisy_counters()
    t = {key: [] for key in calls}
    for _ in range(args.reps):
        for key, fn in calls.items():
            t[key].append(timed(fn))
    c1 = ctx.daisy_counters()
    med = {key: statistics.median(v) for key, v in t.items()}
    per = lambda v: round(1e6 * v / n, 3)      # noqa: E731
    out["sets"].append(dict(image=name, regions=n, us_per_region={key: per(v) for key, v in med.items()},
                            us_per_region_min={key: per(min(v)) for key, v in t.items()},
                            us_per_region_max={key: per(max(v)) for key, v in t.items()},
                            daisy_default_over_sift=round(med["daisy_default"] / med["sift"], 3),
                            daisy_ini_over_sift=round(med["daisy_ini"] / med["sift"], 3), surf_over_sift=round(med["surf"] / med["sift"], 3),
                            daisy_default_minus_patches_us_per_region=per(med["daisy_default"] - med["patches_device"]),
                            sub_batches_per_call=(c1["sub_batches"] - c0["sub_batches"]) / (2 * args.reps)))
    im.free()
    hip.hipFree(dev)

# the functor alone on rows that live in HBM
rng = np.random.default_rng(3)
out["daisy_patches_device"] = []
for key, p in PARAMS.items():
    bd = bounds(p)
    for count in (256, 4096):
        rows = rng.uniform(0, 255, (count, 1681)).astype(np.float32)
        src, dst = dev_alloc(rows.nbytes), dev_alloc(count * 200 * 4)
        assert hip.hipMemcpy(src, rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(rows.nbytes), 1) == 0
        call = lambda: ctx.daisy_patches_device(src.value, count, dst.value, **p)      # noqa: E731
        call()
        ts = [timed(call) for _ in range(args.reps)]
        us = 1e6 * statistics.median(ts) / count
        out["daisy_patches_device"].append(dict(params=key, patches=count, ms=round(1e3 * statistics.median(ts), 4),
                                                ms_min=round(1e3 * min(ts), 4), ms_max=round(1e3 * max(ts), 4), us_per_patch=round(us, 4),
                                                share_of_lds_bound=round(bd["lds_bound_us_per_patch"] / us, 3),
                                                share_of_valu_bound=round(bd["valu_bound_us_per_patch"] / us, 3),
                                                share_of_valu_issued=round(bd["valu_issued_us_per_patch"] / us, 3), **bd))
        hip.hipFree(src)
        hip.hipFree(dst)
print(json.dumps(out))
ctx.close()
