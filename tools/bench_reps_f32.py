#!/usr/bin/env python3
"""One stored float class against 64 partners: the grouped launch sets of stored representations (A) beside one
modsx_match_fginn_f32_device call per partner on the same rows (B).

  A   the query class of one modsx_rep against the class of 64 partner representations through modsx_rep_match_group_f32, four
      partners per call: nothing is packed, two host round trips per group
  B   64 calls of modsx_match_fginn_f32_device on dense device copies of the same rows: both sides packed per call, two host round
      trips per partner -- the path a caller had before float classes could be stored
Rows per side 2 000, 8 000 and 25 000; dim 64, 144 and 200.  Every shape is warmed up with one A and one B, then A and B alternate
--reps (>= 5) times in this process; a timed window is the 64 partners and ends in a device synchronise.  Reported per shape: median
and min .. max of A and of B in ms, the record counts of both (they must agree), and what A added to modsx_fginn32_group_counters.
--group G (default 4) sets the partners per call of A; 1 gives single-problem launch sets from the stored form.
The rows are seeded Gaussian on the device; six queries in ten are noisy copies of a train of partner 0.  There is no fall-back:
without a device the tool fails.  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mods_amd

ROWS = (2000, 8000, 25000)
DIMS = (64, 144, 200)
TYPE_OF_DIM = {64: mods_amd.DESC_SURF, 144: mods_amd.DESC_LIOP, 200: mods_amd.DESC_DAISY}
GROUP = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--partners", type=int, default=64)
    ap.add_argument("--rows", type=int, nargs="*", default=list(ROWS))
    ap.add_argument("--dims", type=int, nargs="*", default=list(DIMS))
    ap.add_argument("--group", type=int, default=GROUP, help="partners per modsx_rep_match_group_f32 call (1 .. 4)")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_reps_f32.py needs a GPU")
    ctx = mods_amd.Context(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    rs = np.random.RandomState(3)
    shapes = [(n, dim) for n in args.rows for dim in args.dims]
    out = []
    for n, dim in shapes:
        typ = TYPE_OF_DIM[dim]
        regs = np.zeros(n, mods_amd.REGION)
        pos = rs.uniform(0, 1000, (n, 2))
        regs["reproj_kp"]["x"], regs["reproj_kp"]["y"] = pos[:, 0], pos[:, 1]
        dense, reps = [], []
        for g in range(args.partners):
            t = torch.randn(n, dim, generator=gen, device="cuda")
            rep = mods_amd.Rep(ctx)
            rep.append_f32(regs, t.cpu().numpy(), 0, typ)
            dense.append(t); reps.append(rep)
        pick = torch.randint(0, n, (n,), generator=gen, device="cuda")
        q = torch.where(torch.rand(n, 1, generator=gen, device="cuda") < 0.6,
                        dense[0][pick] + 0.3 * torch.randn(n, dim, generator=gen, device="cuda"),
                        torch.randn(n, dim, generator=gen, device="cuda")).contiguous()
        rq = mods_amd.Rep(ctx)
        rq.append_f32(regs, q.cpu().numpy(), 0, typ)
        torch.cuda.synchronize()

        def run_a():
            t0 = time.perf_counter()
            nrec = 0
            for i in range(0, len(reps), args.group):
                nrec += sum(len(r) for r in ctx.rep_match_group_f32(rq, reps[i:i + args.group], 0, typ))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, nrec

        def run_b():
            t0 = time.perf_counter()
            nrec = 0
            for t in dense:
                nrec += len(ctx.match_fginn_f32_device(q.data_ptr(), n, t.data_ptr(), n, dim, pos))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, nrec

        run_a(); run_b()                                      # warm-up of this shape: buffers, code objects
        c0 = ctx.fginn32_group_counters()
        a_ms, b_ms, na, nb = [], [], 0, 0
        for _ in range(args.reps):
            ms, na = run_a(); a_ms.append(ms)
            ms, nb = run_b(); b_ms.append(ms)
        c1 = ctx.fginn32_group_counters()
        if na != nb:
            sys.exit("bench_reps_f32.py: A gave %d records, B %d" % (na, nb))
        row = {"rows": n, "dim": dim, "partners": len(reps), "group": args.group, "repeats": args.reps, "records": na,
               "A_ms": float(np.median(a_ms)), "A_min_ms": float(np.min(a_ms)), "A_max_ms": float(np.max(a_ms)),
               "B_ms": float(np.median(b_ms)), "B_min_ms": float(np.min(b_ms)), "B_max_ms": float(np.max(b_ms)),
               "geometry": mods_amd.fginn32_group_geometry(n, [n] * args.group, dim)["per_problem"][0],
               "counters_per_A": {k: (c1[k] - c0[k]) / float(args.reps) for k in c1}}
        row["A_inside_B_span"] = row["B_min_ms"] <= row["A_ms"] <= row["B_max_ms"]
        row["A_slower_than_slowest_B"] = row["A_ms"] > row["B_max_ms"]
        out.append(row)
        print("%6d x %3d  A %9.2f ms (%.2f .. %.2f)   B %9.2f ms (%.2f .. %.2f)" % (n, dim, row["A_ms"], row["A_min_ms"], row["A_max_ms"],
              row["B_ms"], row["B_min_ms"], row["B_max_ms"]), file=sys.stderr, flush=True)
        for r in reps + [rq]:
            r.free()
        del dense, q
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"bench": "reps_f32", "rows": out}))


if __name__ == "__main__":
    main()
