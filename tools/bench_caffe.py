"""Timings of the learned-descriptor front end, in one process:
    python tools/bench_caffe.py [--reps 9]
Regions: those of one image of the benchmark's synthetic pair (1024x768, 5500 blobs) over its 31 views, reprojected to the
original image; det_kp is set to reproj_kp so that extract_patches samples the same frames on the same image.  Colour input: three
planes of that size (the pair's two images and their mean).  Everything writes into device buffers, so no download is timed.
The calls of a group alternate `--reps` times after a warm-up; a call's time is the host clock around it (every entry returns
after its work has finished, the copies are followed by a device synchronise).  Reported per call: median, smallest and largest
time, microseconds per region, and the ratio to a plain device-to-device copy of the bytes the call writes -- the floor for a
kernel that mostly writes.
  caffe_patches at P = 41 (all regions), 65 (at most 8192) and 227 (at most 1024), colour and gray
  extract_patches with fast extraction on the P = 41 regions, and three times that next to the colour blob
  caffe_norm_rows_device (L2, in place) at dim 128 (one row per region) and 4096 (4096 rows)
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
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()

ctx = mods_amd.Context(0)
hip = ctypes.CDLL("libamdhip64.so")
a, b, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=5500, seed=12345)
views = mods_amd.set_vs_pars([1.0], [1.0, 2.0, 4.0, 6.0, 8.0], 120.0, 0.5, 1, [])
planes = [ctx.upload(g) for g in (a, b, ((a + b) / 2).astype(np.float32))]
regs, _ = ctx.detect_describe_views(planes[0], views, mods_amd.default_pair_params(), want_desc=False)
regs = regs.copy()
regs["det_kp"] = regs["reproj_kp"]


def dev_alloc(nbytes):
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
    return p


def copy_call(dst, src, nbytes):
    def f():
        assert hip.hipMemcpy(dst, src, ctypes.c_size_t(nbytes), 3) == 0
        assert hip.hipDeviceSynchronize() == 0
    return f


def run_group(calls):
    """{name: (median, min, max) seconds}: the calls alternate"""
    for fn in calls.values():
        fn()
    t = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def report(t, n, floor):
    return {k: dict(ms=round(1e3 * v[0], 4), ms_min=round(1e3 * v[1], 4), ms_max=round(1e3 * v[2], 4), us_per_region=round(1e6 * v[0] / n, 4),
                    over_copy=round(v[0] / floor, 3)) for k, v in t.items()}


out = {"reps": args.reps, "regions": len(regs), "views": len(views), "patches": [], "norm": []}
for P, cap in ((41, len(regs)), (65, 8192), (227, 1024)):
    r = regs[:cap]
    n, nbytes = len(r), len(r) * 3 * P * P * 4
    dst, src = dev_alloc(nbytes), dev_alloc(nbytes)
    par = mods_amd.caffe_params(patch_size=P)
    calls = {"colour": lambda: ctx.caffe_patches(planes, r, par, out_ptr=dst.value),
             "gray": lambda: ctx.caffe_patches(planes[:1], r, par, out_ptr=dst.value),
             "copy": copy_call(dst, src, nbytes)}
    if P == 41:
        calls["extract_patches_fast"] = lambda: ctx.extract_patches(planes[0], r, fast=1, out_ptr=dst.value)
    t = run_group(calls)
    e = dict(P=P, regions=n, blob_bytes=nbytes, copy_gb_per_s=round(2 * nbytes / t["copy"][0] / 1e9, 1), **report(t, n, t["copy"][0]))
    if P == 41:
        e["colour_over_3_extract_patches"] = round(t["colour"][0] / (3 * t["extract_patches_fast"][0]), 3)
    out["patches"].append(e)
    hip.hipFree(dst)
    hip.hipFree(src)

rng = np.random.default_rng(5)
for dim, n in ((128, len(regs)), (4096, 4096)):
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    buf, src = dev_alloc(rows.nbytes), dev_alloc(rows.nbytes)
    assert hip.hipMemcpy(buf, rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(rows.nbytes), 1) == 0
    # in place: after the first call the rows are normalised rows, which costs the same to normalise again (no NaN: the sum of squares stays positive)
    t = run_group({"l2_in_place": lambda: ctx.caffe_norm_rows_device(buf.value, n, dim, mods_amd.CAFFE_NORM_L2),
                   "copy": copy_call(src, buf, rows.nbytes)})
    out["norm"].append(dict(dim=dim, rows=n, bytes=rows.nbytes, **report(t, n, t["copy"][0])))
    hip.hipFree(buf)
    hip.hipFree(src)
print(json.dumps(out))
for p in planes:
    p.free()
ctx.close()
