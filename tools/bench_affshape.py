"""External affine adaptation (detect_affine_shape_batch on SURF regions) next to the scale-space detector's Baumberg launch
(debug_baumberg on the Hessian-Affine job list) on the same views, in one process:
    python tools/bench_affshape.py [--reps 7] [--views 1,8,31]
Inputs: the 1024x768 synthetic image of bench.py, and synthesised views of it (the first of the view set of tilts 1, 2, 4, 6, 8 at
a rotation step of 45 degrees / tilt, identity included).  Per view count v the first v views give
  external   SURF keypoints (detect_surf_batch) wrapped as regions (surf_regions): one detect_affine_shape_batch call
  hessaff    the scale-space keypoints of the same views (detect_scalespace) on their own pyramid levels, rebuilt from the stage
             taps as tests/test_gpu_baumberg.py does: one debug_baumberg call (production variant)
and the calls alternate `--reps` times.  Reported per side: regions in, regions launched (external: after the up-front border test),
iteration-regions (the iterations the launched regions ran, from the debug entries), converged, the median wall time per call with
the smallest and the largest repetition (job upload, launch, result download and compaction included), and that time per launched
region and per iteration-region.  The external side also reports the ratios it ran at.  Prints one JSON line."""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--views", default="1,8,31")
ap.add_argument("--tilts", default="1,2,4,6,8")
ap.add_argument("--phi", type=float, default=360.0 / 8)
args = ap.parse_args()
counts = [int(v) for v in args.views.split(",")]

ctx = mods_amd.Context(0)
a, _, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
im = ctx.upload(a)
views = mods_amd.set_vs_pars([1.0], [float(t) for t in args.tilts.split(",")], args.phi, 0.5, 1, [])[:max(counts)]
vims = [ctx.synth_view(im, v)[0] for v in views]
hess, aff = mods_amd.default_hessaff_params(), mods_amd.default_affshape_params()

# external side: SURF regions of every view
surf = [mods_amd.surf_regions(k, img_id=i) for i, k in enumerate(ctx.detect_surf_batch(vims))]


def pyramid_jobs(view):
    """(planes, plane_of, xyspd) of one view: its scale-space keypoints and the blur levels their windows read (pyramid.cpp:455-573)"""
    f32 = np.float32
    ss = ctx.detect_scalespace(view, hess)
    first = ctx.gaussian_blur(view, float(np.sqrt(f32(hess.initialSigma) * f32(hess.initialSigma) - f32(0.5) * f32(0.5))))
    min_size = 2 * hess.border + 2
    planes, index, octave = [], {}, 0
    while first.shape[0] > min_size and first.shape[1] > min_size:
        fl = ctx.upload(first)
        blurs, _ = ctx.octave_levels(fl, hess)
        fl.free()
        for level in range(1, hess.numberOfScales + 1):
            index[(octave, level)] = len(planes)
            planes.append(ctx.upload(blurs[level - 1]))
        seed = ctx.upload(blurs[hess.numberOfScales])
        first = ctx.resize_half(seed)
        seed.free()
        octave += 1
    plane_of = np.array([index[(int(o), int(l))] for o, l in zip(ss["octave"], ss["level"])], np.int32)
    return planes, plane_of, np.stack([ss["x"], ss["y"], ss["s"], ss["pixelDistance"]], 1)


hjobs = [pyramid_jobs(v) for v in vims]


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def alternate(calls):
    for fn in calls.values():
        fn()                                                     # warm-up: buffers, tables
    t = {key: [] for key in calls}
    for _ in range(args.reps):
        for key, fn in calls.items():
            t[key].append(timed(fn))
    return {key: (statistics.median(v), min(v), max(v)) for key, v in t.items()}


def passes(iters, ok_launched, max_iter):
    """iterations a launched region ran: the loop counter at its break + 1, maxIterations when the loop ran out"""
    it = iters[ok_launched]
    return int(np.where(it >= max_iter, max_iter, it + 1).sum())


def side(t, regions, launched, iter_regions, converged, **more):
    med, lo, hi = t
    us = lambda v: round(1e6 * v, 4)      # noqa: E731
    return dict(regions=regions, launched=launched, iteration_regions=iter_regions, converged=converged, ms=round(1e3 * med, 4),
                ms_min=round(1e3 * lo, 4), ms_max=round(1e3 * hi, 4), us_per_launched=us(med / max(1, launched)),
                us_per_iteration_region=us(med / max(1, iter_regions)), **more)


out = {"reps": args.reps, "image": [a.shape[1], a.shape[0]], "calls": []}
for v in counts:
    ims, regs = vims[:v], surf[:v]
    planes, plane_of, xyspd = [], [], []
    for p, po, xy in hjobs[:v]:
        plane_of.append(po + len(planes))
        planes += p
        xyspd.append(xy)
    plane_of, xyspd = np.concatenate(plane_of), np.concatenate(xyspd)
    variant = mods_amd.baumberg_production_variant(hess.smmWindowSize)
    t = alternate({"external": lambda: ctx.detect_affine_shape_batch(ims, regs, aff),
                   "hessaff": lambda: ctx.debug_baumberg(planes, plane_of, xyspd, hess, variant=variant)})
    de = ctx.debug_affine_shape(ims, regs, aff)
    dh = ctx.debug_baumberg(planes, plane_of, xyspd, hess, variant=variant)
    ratios = np.concatenate([mods_amd.affshape_jobs(r, i.cols, i.rows)["ratio"] for r, i in zip(regs, ims)])[~de["border"]]
    out["calls"].append(dict(
        views=v,
        external=side(t["external"], len(de["ok"]), de["launched"], passes(de["iters"], ~de["border"], aff.maxIterations), int(de["ok"].sum()),
                      ratio_min=round(float(ratios.min()), 3), ratio_median=round(float(np.median(ratios)), 3),
                      ratio_max=round(float(ratios.max()), 3), geometry=de["geometry"]),
        hessaff=side(t["hessaff"], len(dh["ok"]), len(dh["ok"]), passes(dh["iters"], np.ones(len(dh["ok"]), bool), hess.maxIterations),
                     int(dh["ok"].sum()), geometry=dh["geometry"])))
out["affshape_counters"] = ctx.affshape_counters()
# last, because profiling leaves the context's queue slower: the external launch alone, by the stream's events
ctx.profile(True)
for v, call in zip(counts, out["calls"]):
    before = ctx.kernel_stats()["baumberg"]
    ctx.detect_affine_shape_batch(vims[:v], surf[:v], aff)
    after = ctx.kernel_stats()["baumberg"]
    assert after["launches"] == before["launches"] + 1
    call["external"]["kernel_ms"] = round(after["ms"] - before["ms"], 4)
ctx.profile(False)
print(json.dumps(out))
for p, _, _ in hjobs:
    for q in p:
        q.free()
for v in vims:
    v.free()
im.free()
ctx.close()
