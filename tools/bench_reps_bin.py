#!/usr/bin/env python3
"""One stored binary class against 64 partners: the grouped Hamming launch sets of stored representations (A) beside one
modsx_match_hamming_device call per partner on the same rows (B).

  A   the query class of one modsx_rep against the class of 64 partner representations through modsx_rep_match_group_hamming, four
      partners per call (16 launch sets): nothing is packed, one host round trip per group
  B   64 calls of modsx_match_hamming_device on dense device copies of the same rows: both sides packed per call, one host round
      trip per partner -- the path a caller had before binary classes could be stored
Rows per side 2 000, 8 000 and 25 000; 32 and 64 bytes per row.  Every shape is warmed up with three A and three B, then A and B
alternate --reps (>= 11) times in this process; a timed window is the 64 partners (wall time) and ends in a device synchronise.
Reported per shape: median and min .. max of A and of B in ms, the record counts of both (they must agree), the tile / splits /
workgroups of one partner, and what one window of A and one of B added to modsx_hamming_group_counters.
--group G (default 4) sets the partners per call of A; 1 gives single-problem launch sets from the stored form.
The rows are seeded random bytes made on the device; six queries in ten are a train of partner 0 with some bits flipped.  There is
no fall-back: without a device the tool fails.  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mods_amd

ROWS = (2000, 8000, 25000)
NBYTES = (32, 64)
GROUP = 4
THRESHOLD = 64.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--partners", type=int, default=64)
    ap.add_argument("--rows", type=int, nargs="*", default=list(ROWS))
    ap.add_argument("--nbytes", type=int, nargs="*", default=list(NBYTES))
    ap.add_argument("--group", type=int, default=GROUP, help="partners per modsx_rep_match_group_hamming call (1 .. 4)")
    args = ap.parse_args()
    if args.reps < 11:
        ap.error("--reps must be at least 11")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_reps_bin.py needs a GPU")
    ctx = mods_amd.Context(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    det, typ = mods_amd.DET_ORB, mods_amd.DESC_ORB
    out = []
    for n in args.rows:
        for nbytes in args.nbytes:
            regs = np.zeros(n, mods_amd.REGION)
            dense, reps = [], []
            for g in range(args.partners):
                t = torch.randint(0, 256, (n, nbytes), generator=gen, device="cuda", dtype=torch.uint8).contiguous()
                rep = mods_amd.Rep(ctx)
                rep.append_bin_device(regs, t.data_ptr(), nbytes, det, typ)
                dense.append(t); reps.append(rep)
            pick = torch.randint(0, n, (n,), generator=gen, device="cuda")
            noise = (torch.rand(n, nbytes, generator=gen, device="cuda") < 0.1).to(torch.uint8) << 3      # bit 3 of one byte in ten
            q = torch.where(torch.rand(n, 1, generator=gen, device="cuda") < 0.6, dense[0][pick] ^ noise,
                            torch.randint(0, 256, (n, nbytes), generator=gen, device="cuda", dtype=torch.uint8)).contiguous()
            rq = mods_amd.Rep(ctx)
            rq.append_bin_device(regs, q.data_ptr(), nbytes, det, typ)
            torch.cuda.synchronize()

            def run_a():
                t0 = time.perf_counter()
                nrec = 0
                for i in range(0, len(reps), args.group):
                    nrec += sum(len(r) for r in ctx.rep_match_group_hamming(rq, reps[i:i + args.group], det, typ, THRESHOLD))
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, nrec

            def run_b():
                t0 = time.perf_counter()
                nrec = 0
                for t in dense:
                    nrec += len(ctx.match_hamming_device(q.data_ptr(), n, t.data_ptr(), n, nbytes, THRESHOLD))
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, nrec

            for _ in range(args.warmup):                          # warm-up of this shape: buffers, code objects
                run_a(); run_b()
            a_ms, b_ms, na, nb = [], [], 0, 0
            ca = {k: 0 for k in mods_amd.HAMMING_GROUP_COUNTERS}
            cb = dict(ca)
            for _ in range(args.reps):
                c0 = ctx.hamming_group_counters()
                ms, na = run_a(); a_ms.append(ms)
                c1 = ctx.hamming_group_counters()
                ms, nb = run_b(); b_ms.append(ms)
                c2 = ctx.hamming_group_counters()
                for k in ca:
                    ca[k] += c1[k] - c0[k]; cb[k] += c2[k] - c1[k]
            if na != nb:
                sys.exit("bench_reps_bin.py: A gave %d records, B %d" % (na, nb))
            geo = mods_amd.hamming_group_geometry(n, [n] * args.group, nbytes)
            tiles, S, tps = geo["per_problem"][0]
            row = {"rows": n, "nbytes": nbytes, "partners": len(reps), "group": args.group, "repeats": args.reps, "records": na,
                   "A_ms": float(np.median(a_ms)), "A_min_ms": float(np.min(a_ms)), "A_max_ms": float(np.max(a_ms)),
                   "B_ms": float(np.median(b_ms)), "B_min_ms": float(np.min(b_ms)), "B_max_ms": float(np.max(b_ms)),
                   "tile": geo["tile"], "S": S, "tiles_per_split": tps, "workgroups_per_partner": geo["gx"] * S,
                   "counters_per_A": {k: v / float(args.reps) for k, v in ca.items()},
                   "counters_per_B": {k: v / float(args.reps) for k, v in cb.items()}}
            row["A_median_not_above_slowest_B"] = row["A_ms"] <= row["B_max_ms"]
            out.append(row)
            print("%6d x %2d B  A %9.2f ms (%.2f .. %.2f)   B %9.2f ms (%.2f .. %.2f)   tile %d S %d wg %d" % (
                n, nbytes, row["A_ms"], row["A_min_ms"], row["A_max_ms"], row["B_ms"], row["B_min_ms"], row["B_max_ms"], geo["tile"], S,
                geo["gx"] * S), file=sys.stderr, flush=True)
            for r in reps + [rq]:
                r.free()
            del dense, q
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"bench": "reps_bin", "rows": out}))


if __name__ == "__main__":
    main()
