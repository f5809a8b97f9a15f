"""CLAHE on the device next to a plain device copy of the same images, in one process:
    python tools/bench_clahe.py [--reps 15] [--batch 64]
Configurations: one 1024x768 image, one 1920x1080 image, and a batch of --batch of each through clahe_batch (one launch set),
at the drivers' parameters (clip 4, 8 x 8, variant 0), out of place into preallocated images.  Per configuration the CLAHE call
and the yardstick alternate --reps times after a warm-up of both:
  clahe   the HIP-event times of the three launches (k_clahe_hist, k_clahe_lut, k_clahe_apply) as the library records them
          around its own launches under profile(True), and the host's wall time of the whole call (table upload, three launches,
          the wait)
  copy    torch's device-to-device copy of as many floats (4 B read + 4 B written per pixel), timed by events on its stream
Reported: median (min .. max) per launch; the bytes the three passes need (12 B/px: 4 read by the histogram pass, 4 read and 4
written by the pixel pass) and the bytes they move counting the strip partials, the LUT table and its per-workgroup staging, from
clahe_geometry; bytes needed over the summed launch time, and per pass over its own time, next to the copy's rate.
Prints one JSON line."""
import argparse
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
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_clahe.py needs the GPU: no time is reported without one")

ctx = mods_amd.Context(0)
ctx.profile(True)


def stats(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def moved_bytes(rows, cols):
    """bytes one image moves through the three launches, from the library's own geometry (8 x 8 tiles)"""
    g = mods_amd.clahe_geometry(rows, cols)
    px, tiles = rows * cols, 64
    partials = tiles * g["strips"] * 1024
    return dict(needed=12 * px,
                hist=4 * px + partials,                          # the source once, the strip partials out
                lut=partials + tiles * 256,                      # the partials back in, the LUTs out
                apply=8 * px + g["apply_blocks"] * tiles * 256)  # source in, result out, the LUT table staged once per workgroup


_base = {}


def run(name, rows, cols, n):
    if (rows, cols) not in _base:
        _base[(rows, cols)] = synthetic.blob_image(rows, cols, int(4000 * rows * cols / (768 * 1024)), 12345)
    base = _base[(rows, cols)]
    src = [ctx.upload(np.roll(base, 17 * i, axis=1)) for i in range(n)]
    dst = [ctx.upload(np.zeros((rows, cols), np.float32)) for _ in range(n)]
    ta = torch.rand(n * rows * cols, device="cuda")
    tb = torch.empty_like(ta)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def clahe():
        t = time.perf_counter()
        if n == 1:
            ctx.clahe(src[0], out=dst[0])
        else:
            ctx.clahe_batch(src, out=dst)
        return (time.perf_counter() - t) * 1e3, ctx.clahe_last_ms()

    def copy():
        e0.record()
        tb.copy_(ta)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):
        clahe(), copy()
    wall, hist, lut, app, cp = [], [], [], [], []
    for _ in range(args.reps):
        w, (h, l, a) = clahe()
        wall.append(w); hist.append(h); lut.append(l); app.append(a)
        cp.append(copy())
    for im in src + dst:
        im.free()
    mv = moved_bytes(rows, cols)
    px = n * rows * cols
    launches = [h + l + a for h, l, a in zip(hist, lut, app)]
    gbs = lambda b, ms: round(b / (ms * 1e-3) / 1e9, 1)     # noqa: E731
    return dict(config=name, images=n, rows=rows, cols=cols, geometry=mods_amd.clahe_geometry(rows, cols) | dict(lut_scale=None),
                ms=dict(hist=stats(hist), lut=stats(lut), apply=stats(app), launches=stats(launches), call_wall=stats(wall), copy=stats(cp)),
                bytes_per_px=dict(needed=12.0, moved=round((mv["hist"] + mv["lut"] + mv["apply"]) / (rows * cols), 3),
                                  hist=round(mv["hist"] / (rows * cols), 3), lut=round(mv["lut"] / (rows * cols), 3),
                                  apply=round(mv["apply"] / (rows * cols), 3), copy=8.0),
                gb_per_s=dict(needed_over_launches=gbs(12 * px, statistics.median(launches)),
                              hist=gbs(n * mv["hist"], statistics.median(hist)), apply=gbs(n * mv["apply"], statistics.median(app)),
                              copy=gbs(8 * px, statistics.median(cp))))


out = [run("1024x768", 768, 1024, 1), run("1920x1080", 1080, 1920, 1),
       run("1024x768 x%d" % args.batch, 768, 1024, args.batch), run("1920x1080 x%d" % args.batch, 1080, 1920, args.batch)]
ctx.close()
print(json.dumps(dict(reps=args.reps, results=out)))
