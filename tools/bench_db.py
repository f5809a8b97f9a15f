#!/usr/bin/env python3
"""Timing of the database pass of MatchFlannFGINNPlusDB (kernels_dbnn.hip k_dbnn_min, kernel class `match_db`).

  kernel      k_dbnn_min at --queries x --rows (default 4 096 x 2^20: every query selected, through modsx_db_nearest) against
              k_match_sweep1 (class `match_sweep1`, through modsx_match_fginn_device) on the SAME problem -- the same int8
              contraction with a heavier epilogue -- in one process, alternating, each warmed up, --reps repeats (>= 7): medians,
              spread, the achieved int8 rate 2 n rows 128 / time and its share of the 5 POP/s peak.  A second point at
              --queries2 (25 600, the ratio >= 1 use) is reported for k_dbnn_min alone.
  --e2e       the headline shape (31 views, 1024x768, 16 contexts, modsx_match_pairs_views) with and without the database
              attached, alternating: pairs/s and the match_db share of the kernel time of a pair (report only).
Device-event times per kernel class (modsx_profile); the descriptors are seeded SIFT-like rows (sparse prototypes plus jitter).
Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mods_amd

PEAK_INT8 = 5.0e15      # dense int8 peak the project's figures use


def sift_like(rs, protos, n, jitter):
    out = np.empty((n, 128), np.uint8)
    for s in range(0, n, 1 << 16):
        c = min(1 << 16, n - s)
        p = protos[rs.randint(0, len(protos), c)].astype(np.int16)
        out[s:s + c] = np.clip(p + rs.randint(-jitter, jitter + 1, (c, 128), dtype=np.int16), 0, 255)
    return out


def stats(ms, work):
    ms = np.sort(np.array(ms))
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms[0]), "max_ms": float(ms[-1]), "spread_pct": 100.0 * float(ms[-1] - ms[0]) / med,
            "repeats": len(ms), "int8_ops_per_s": work / (med * 1e-3), "share_of_5_POPs_peak_pct": 100.0 * work / (med * 1e-3) / PEAK_INT8}


def kernel_part(args):
    import torch
    ctx = mods_amd.Context(0)
    rs = np.random.RandomState(7)
    protos = (rs.randint(0, 256, (4096, 128)) * (rs.rand(4096, 128) < 0.35)).astype(np.uint8)
    rows = sift_like(rs, protos, args.rows, 6)
    db = ctx.db_create(rows)
    t2 = torch.from_numpy(rows).cuda()
    pos2 = rs.uniform(0, 1000, (args.rows, 2))
    out = {"rows": args.rows}

    def queries(n):
        return sift_like(rs, protos, n, 40)

    def time_db(q):
        ctx.profile(True)
        ctx.db_nearest(db, q)
        return ctx.kernel_stats()["match_db"]["ms"]

    def time_sweep1(tq, n):
        ctx.profile(True)
        ctx.match_fginn_device(tq.data_ptr(), n, t2.data_ptr(), args.rows, pos2)
        return ctx.kernel_stats()["match_sweep1"]["ms"]

    n = args.queries
    q = queries(n).astype(np.float32)
    tq = torch.from_numpy(q.astype(np.uint8)).cuda()
    for _ in range(args.warmup):
        time_db(q); time_sweep1(tq, n)
    a, b = [], []
    for _ in range(args.reps):                      # alternating
        a.append(time_db(q)); b.append(time_sweep1(tq, n))
    work = 2.0 * n * args.rows * 128
    out["queries"] = n
    out["k_dbnn_min"] = stats(a, work)
    out["k_match_sweep1"] = stats(b, work)
    ratio = out["k_dbnn_min"]["median_ms"] / out["k_match_sweep1"]["median_ms"]
    out["dbnn_over_sweep1"] = ratio
    spread = max(out["k_dbnn_min"]["spread_pct"], out["k_match_sweep1"]["spread_pct"])
    out["target"] = "k_dbnn_min <= 1.10 x k_match_sweep1"
    out["verdict"] = ("spread of the repeats (%.1f %%) exceeds the 10 %% margin: raise --reps" % spread) if spread > 10.0 else \
        ("met" if ratio <= 1.10 else "missed")
    if args.queries2:
        n2 = args.queries2
        q2 = queries(n2).astype(np.float32)
        for _ in range(args.warmup):
            time_db(q2)
        out["report_only_%d_queries" % n2] = stats([time_db(q2) for _ in range(args.reps)], 2.0 * n2 * args.rows * 128)
    db.free()
    ctx.close()
    return out


def e2e_part(args):
    from mods_amd import synthetic
    ctxs = [mods_amd.Context(0) for _ in range(args.workers)]
    rs = np.random.RandomState(7)
    protos = (rs.randint(0, 256, (4096, 128)) * (rs.rand(4096, 128) < 0.35)).astype(np.uint8)
    db = ctxs[0].db_create(sift_like(rs, protos, args.rows, 6))
    views = mods_amd.set_vs_pars([1.0], [1.0, 2.0, 4.0, 6.0, 8.0], 120.0, 0.2, 1, [])
    par = mods_amd.default_pair_params()
    pairs = [synthetic.make_pair(rows=768, cols=1024, nblobs=2000, seed=100 + i) for i in range(4)]
    ims = [(ctxs[0].upload(a), ctxs[0].upload(b)) for a, b, _ in pairs]
    i1 = [ims[i % len(ims)][0] for i in range(args.pairs)]
    i2 = [ims[i % len(ims)][1] for i in range(args.pairs)]

    def run(with_db, profile=False):
        for c in ctxs:
            c.set_fginn_db(db if with_db else None)
            c.profile(profile)
        t0 = time.time()
        res = mods_amd.match_pairs_views(ctxs, i1, i2, views, par, arrays=False)
        dt = time.time() - t0
        return len(res) / dt, res

    for w in (False, True):
        run(w)
    rate = {False: [], True: []}
    for _ in range(args.e2e_reps):                  # alternating
        for w in (False, True):
            rate[w].append(run(w)[0])
    # the match_db share of a pair's kernel time: a profiled run of its own (event timing slows the host)
    _, res = run(True, profile=True)
    tot, dbms = 0.0, 0.0
    for c in ctxs:
        st = c.kernel_stats()
        dbms += st["match_db"]["ms"]
        tot += sum(v["ms"] for k, v in st.items() if k != "match_sweep1")      # match_sweep1 is part of match_fginn
    _, res0 = run(False)
    for c in ctxs:
        c.set_fginn_db(None)
    out = {"views": len(views), "contexts": len(ctxs), "pairs_per_call": args.pairs, "rows": args.rows,
           "pairs_per_s_without_db": {"median": float(np.median(rate[False])), "min": min(rate[False]), "max": max(rate[False])},
           "pairs_per_s_with_db": {"median": float(np.median(rate[True])), "min": min(rate[True]), "max": max(rate[True])},
           "match_db_ms_per_pair": dbms / args.pairs, "kernel_ms_per_pair": tot / args.pairs,
           "match_db_share_of_kernel_time_pct": 100.0 * dbms / tot if tot else None,
           "tentatives_per_pair_without_db": float(np.mean([r["n_tentatives"] for r in res0])),
           "tentatives_per_pair_with_db": float(np.mean([r["n_tentatives"] for r in res]))}
    db.free()
    for x, y in ims:
        x.free(); y.free()
    for c in ctxs:
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--queries2", type=int, default=25600)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--e2e-reps", type=int, default=3)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps must be at least 7")
    out = {"tool": "bench_db"}
    if not args.no_kernel:
        out["kernel"] = kernel_part(args)
    if args.e2e:
        out["end_to_end"] = e2e_part(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
