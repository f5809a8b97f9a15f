"""SURF detector timings next to the Hessian-Affine detector on the same inputs, in one process:
    python tools/bench_surfdet.py [--reps 7] [--views 31]
Inputs: the 1024x768 synthetic image of tools/bench_liop.py, and `--views` synthesised views of it (the first of the view set of
tilts 1, 2, 4, 6, 8 at a rotation step of 45 degrees / tilt, identity included).  Per input the calls alternate `--reps` times:
  single   detect_surf(image)                      against  detect_affine_keypoints(image)
  batch    detect_surf_batch(views): one call      against  detect_affine_keypoints(view) per view, one after the other
and the median wall time per call is reported with the smallest and the largest of the repetitions (downloads included).  The
launches per call are what the engine issues for one launch set of the SURF detector: rows, columns, responses, scan, offsets and
-- when there is an extremum -- emit; a call of more than 32 images runs one such set per 32.  Prints one JSON line."""
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
hess, surf = mods_amd.default_hessaff_params(), mods_amd.surfdet_params()


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


def surf_launches(n_images, found):
    sets = (n_images + 31) // 32
    return sets * (5 + (1 if found else 0))


out = {"reps": args.reps, "views": len(vims), "image": [a.shape[1], a.shape[0]]}
c0 = ctx.surfdet_counters()
n_surf, n_hess = len(ctx.detect_surf(im, surf)), len(ctx.detect_affine_keypoints(im, hess))
out["single"] = dict(points_surf=n_surf, keypoints_hessaff=n_hess, surf_launches_per_call=surf_launches(1, n_surf),
                     **alternate({"detect_surf": lambda: ctx.detect_surf(im, surf),
                                  "detect_affine_keypoints": lambda: ctx.detect_affine_keypoints(im, hess)}))
n_surf_b = sum(len(k) for k in ctx.detect_surf_batch(vims, surf))
n_hess_b = sum(len(ctx.detect_affine_keypoints(v, hess)) for v in vims)
out["batch"] = dict(points_surf=n_surf_b, keypoints_hessaff=n_hess_b, surf_launches_per_call=surf_launches(len(vims), n_surf_b),
                    view_sizes=sorted({(v.cols, v.rows) for v in vims})[:4],
                    **alternate({"detect_surf_batch": lambda: ctx.detect_surf_batch(vims, surf),
                                 "detect_affine_keypoints_each": lambda: [ctx.detect_affine_keypoints(v, hess) for v in vims]}))
c1 = ctx.surfdet_counters()
out["surfdet_counters"] = {k: c1[k] - c0[k] for k in c1}
print(json.dumps(out))
for v in vims:
    v.free()
im.free()
ctx.close()
