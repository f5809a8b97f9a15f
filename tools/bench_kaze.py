"""KAZE detector timings next to the Hessian-Affine and SURF detectors on the same inputs, in one process:
    python tools/bench_kaze.py [--reps 7] [--views 31]
Inputs: the 1024x768 synthetic image of tools/bench_surfdet.py, and `--views` synthesised views of it (the first of the view set
of tilts 1, 2, 4, 6, 8 at a rotation step of 45 degrees / tilt, identity included).  Per input the calls alternate `--reps` times:
  single   detect_kaze(image)                 against  detect_affine_keypoints(image) and detect_surf(image)
  batch    detect_kaze_batch(views): one call against  detect_affine_keypoints(view) per view and detect_surf_batch(views)
and the median wall time per call is reported with the smallest and the largest of the repetitions (downloads included).  From
the detector's counters: kernel launches, diffusion-step launches and host waits per call, and the share of the call the host
spends in the two filter passes of Find_Scale_Space_Extrema and in the refinement loop.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mods_amd  # noqa: E402
from mods_amd import synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--views", type=int, default=31)
ap.add_argument("--tilts", default="1,2,4,6,8")
ap.add_argument("--phi", type=float, default=360.0 / 8)
args = ap.parse_args()

ctx = mods_amd.Context(0)
a, _, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
im = ctx.upload(a)
views = mods_amd.set_vs_pars([1.0], [float(t) for t in args.tilts.split(",")], args.phi, 0.5, 1, [])[:args.views]
vims = [ctx.synth_view(im, v)[0] for v in views]
hess, surf, kaze = mods_amd.default_hessaff_params(), mods_amd.surfdet_params(), mods_amd.kaze_params()


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
    ms = lambda v: round(1e3 * v, 4)      # noqa: E731
    return {key: dict(ms=ms(statistics.median(v)), ms_min=ms(min(v)), ms_max=ms(max(v))) for key, v in t.items()}


def per_call(fn):
    """the detector's counters of one call"""
    c0 = ctx.kaze_counters()
    fn()
    c1 = ctx.kaze_counters()
    return {k: c1[k] - c0[k] for k in c1}


out = {"reps": args.reps, "views": len(vims), "image": [a.shape[1], a.shape[0]]}
one = per_call(lambda: ctx.detect_kaze(im, kaze))
res = alternate({"detect_kaze": lambda: ctx.detect_kaze(im, kaze),
                 "detect_affine_keypoints": lambda: ctx.detect_affine_keypoints(im, hess),
                 "detect_surf": lambda: ctx.detect_surf(im, surf)})
out["single"] = dict(counters=one, filter_share=round(one["filter_us"] / (1e3 * res["detect_kaze"]["ms"]), 4), **res)
many = per_call(lambda: ctx.detect_kaze_batch(vims, kaze))
res = alternate({"detect_kaze_batch": lambda: ctx.detect_kaze_batch(vims, kaze),
                 "detect_affine_keypoints_each": lambda: [ctx.detect_affine_keypoints(v, hess) for v in vims],
                 "detect_surf_batch": lambda: ctx.detect_surf_batch(vims, surf)})
out["batch"] = dict(counters=many, filter_share=round(many["filter_us"] / (1e3 * res["detect_kaze_batch"]["ms"]), 4),
                    view_sizes=sorted({(v.cols, v.rows) for v in vims})[:4], **res)
print(json.dumps(out))
for v in vims:
    v.free()
im.free()
ctx.close()
