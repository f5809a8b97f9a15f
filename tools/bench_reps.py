#!/usr/bin/env python3
"""Timing of the stored image representations (engine_reps.hip): one query image against N partners.

  end to end  the headline shape (1024x768, 31 views, the headline's parameters) with ONE query against --partners distinct
              partner images on --workers contexts: modsx_match_one_to_many (single step; describes N + 1 images) against the N
              pairs (query, partner_i) through modsx_match_pairs_views (describes 2 N images), alternating in one process, each
              warmed up.  The results must be identical.  Wall time per call: median and min-max of --reps repeats.
  match only  the N + 1 representations are kept.  Device-event time (kernel class match_fginn, modsx_profile) per problem of
                packed    modsx_rep_match_fginn, one partner per call: the train half of the pack is switched off
                per_call  modsx_match_fginn_device on the same descriptors and positions, one problem per call (the public device
                          matcher takes one problem per call): the train half runs in every call
                grouped   modsx_match_reps over all partners on one context: four pre-packed problems per launch set
              alternating, each warmed up; the pack share removed = 1 - packed / per_call.
Inputs are seeded (mods_amd.synthetic.make_pairs, the seeds of bench.py).  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mods_amd
from mods_amd import synthetic


def stats(v):
    v = np.sort(np.array(v, np.float64))
    med = float(np.median(v))
    return {"median": med, "min": float(v[0]), "max": float(v[-1]), "spread_pct": 100.0 * float(v[-1] - v[0]) / med, "repeats": len(v)}


def same_result(a, b):
    if any(a[k] != b[k] for k in ("n_regions", "n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples")):
        return False
    return a["H"].tobytes() == b["H"].tobytes() and a["tentatives"].tobytes() == b["tentatives"].tobytes() and \
        np.array_equal(a["verified"], b["verified"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--partners", type=int, default=64)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--rows", type=int, default=768)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--blobs", type=int, default=5500, help="blobs per 1024x768 (the headline's density)")
    ap.add_argument("--tilts", type=str, default="1,2,4,6,8")
    ap.add_argument("--phi", type=float, default=120.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--match-reps", type=int, default=5)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-match", action="store_true")
    args = ap.parse_args()
    n = args.partners
    nblobs = int(args.blobs * args.rows * args.cols / (768.0 * 1024))
    ctxs = [mods_amd.Context(0) for _ in range(max(1, args.workers))]
    ctx = ctxs[0]
    par = mods_amd.default_pair_params(ransac_seed=1)
    views = mods_amd.set_vs_pars([1.0], [float(t) for t in args.tilts.split(",")], args.phi, 0.2, 1, [])
    specs = [(args.rows, args.cols, nblobs, 12345 + 17 * i, 12345 + 17 * i + 42000) for i in range(n)]
    host = synthetic.make_pairs(specs, procs=16, as_u8=True)
    query = ctx.upload(host[0][0])
    partners = [ctx.upload(b) for _, b, _ in host]          # partner 0 shows the query's scene, the others do not
    out = {"tool": "bench_reps", "views": len(views), "contexts": len(ctxs), "partners": n, "rows": args.rows, "cols": args.cols,
           "blobs": nblobs}
    steps = [(views, par.match_ratio)]

    if not args.no_e2e:
        def new(arrays=False):
            t0 = time.perf_counter()
            r, _ = mods_amd.match_one_to_many(ctxs, query, partners, steps, par, min_matches=2 ** 30, arrays=arrays)
            return (time.perf_counter() - t0) * 1e3, r

        def base(arrays=False):
            t0 = time.perf_counter()
            r = mods_amd.match_pairs_views(ctxs, [query] * n, partners, views, par, arrays=arrays)
            return (time.perf_counter() - t0) * 1e3, r

        _, rn = new(True)
        _, rb = base(True)
        identical = all(same_result(a, b) for a, b in zip(rn, rb))
        for _ in range(max(0, args.warmup - 1)):
            new(); base()
        tn, tb = [], []
        for _ in range(args.reps):                          # alternating
            tn.append(new()[0]); tb.append(base()[0])
        sn, sb = stats(tn), stats(tb)
        out["end_to_end"] = {"results_identical": bool(identical), "one_to_many_ms": sn, "pairs_views_ms": sb,
                             "images_described": {"one_to_many": n + 1, "pairs_views": 2 * n},
                             "speedup_median": sb["median"] / sn["median"],
                             "regions_query": rn[0]["n_regions"][0], "verified_partner0": rn[0]["n_verified"],
                             "requirement": "one_to_many median <= pairs_views median + (pairs_views max - min)",
                             "verdict": "met" if identical and sn["median"] <= sb["median"] + (sb["max"] - sb["min"]) else "missed"}

    if not args.no_match:
        import torch
        rq = mods_amd.Rep(ctx)
        rq.add_views(query, views, par)
        reps = []
        for i, im in enumerate(partners):
            reps.append(mods_amd.Rep(ctx))
            reps[-1].add_views(im, views, par, ctx=ctxs[i % len(ctxs)])
        qd = torch.from_numpy(rq.regions()[1]).cuda()
        dev = []
        for r in reps:
            rr, dd = r.regions()
            dev.append((torch.from_numpy(dd).cuda(), np.ascontiguousarray(np.stack([rr["reproj_kp"]["x"], rr["reproj_kp"]["y"]], 1)), len(rr)))
        torch.cuda.synchronize()
        n1 = len(qd)
        ratio, cd, nn = par.match_ratio, par.contradDist, par.nn

        def packed():
            ctx.profile(True)
            got = [ctx.rep_match_fginn(rq, r, 0, 1, ratio, cd, nn) for r in reps]
            return ctx.kernel_stats()["match_fginn"]["ms"] * 1e3 / n, got

        def per_call():
            ctx.profile(True)
            got = [ctx.match_fginn_device(qd.data_ptr(), n1, d.data_ptr(), m, pos, ratio, cd, nn) for d, pos, m in dev]
            return ctx.kernel_stats()["match_fginn"]["ms"] * 1e3 / n, got

        def grouped():
            ctx.profile(True)
            mods_amd.match_reps([ctx], rq, reps, par, arrays=False)
            return ctx.kernel_stats()["match_fginn"]["ms"] * 1e3 / n

        _, ga = packed()
        _, gb = per_call()
        same = all(a.tobytes() == b.tobytes() for a, b in zip(ga, gb))
        for _ in range(max(0, args.warmup - 1)):
            packed(); per_call(); grouped()
        ta, tb, tg = [], [], []
        for _ in range(args.match_reps):                    # alternating
            ta.append(packed()[0]); tb.append(per_call()[0]); tg.append(grouped())
        sa, sb, sg = stats(ta), stats(tb), stats(tg)
        out["match_only"] = {"results_identical": bool(same), "queries": n1, "trains_mean": float(np.mean([m for _, _, m in dev])),
                             "packed_us_per_problem": sa, "per_call_us_per_problem": sb, "grouped_us_per_problem": sg,
                             "pack_share_removed_pct": 100.0 * (1.0 - sa["median"] / sb["median"]),
                             "requirement": "packed median <= per_call median + (per_call max - min)",
                             "verdict": "met" if same and sa["median"] <= sb["median"] + (sb["max"] - sb["min"]) else "missed"}
        for r in reps + [rq]:
            r.free()
    print(json.dumps(out))
    for im in partners + [query]:
        im.free()
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
