#!/usr/bin/env python3
"""Timing of the f32 FGINN matcher's launches (kernels_fginn32.hip) with HIP events; at dim = 128 beside the int8 matcher on the same
problem.

Sizes 2 000 x 2 000, 8 192 x 8 192 and 24 123 x 23 632, dim 64, 128 and 256.  Per size and width: --warmup calls, then --reps
(>= 20) timed repetitions.  At dim = 128 the rows hold 6-bit integers and the repetitions ALTERNATE modsx_match_fginn_f32_device with
modsx_match_fginn_device on the same rows (as u8) in this process, so the two share the machine's state; medians are reported.
  measured   pack_us (the two k_f32_pack launches), search_us (k_f32_topk + k_f32_merge) -- device events under modsx_profile; at
             dim = 128 fginn_us (every launch of the int8 matcher, class match_fginn) and sweep1_us (its contraction launch alone)
  computed   pairs_per_s = n1 n2 / search time; valu_bound_us = n1 n2 / 64 x VALU_PER_PAIR[DK] wave instructions x 2 cycles each /
             (256 CUs x 4 SIMDs x 2.4 GHz); bound_fraction = valu_bound_us / search_us.  VALU_PER_PAIR is the vector-instruction count
             of the sweep loop of k_f32_topk<DK> per (query, train), counted in the kernel's ISA.
The float rows are seeded Gaussian (queries: noisy copies of trains and unrelated rows).  Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mods_amd

SIZES = ((2000, 2000), (8192, 8192), (24123, 23632))
DIMS = (64, 128, 256)
VALU_PER_PAIR = {32: 100, 64: 195, 128: 387, 192: 551, 256: 744}
SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 256 * 4, 2.4e9, 2.0


def valu_bound_us(n1, n2, DK):
    return n1 * n2 / 64.0 * VALU_PER_PAIR[DK] * CYCLES_PER_VALU / (SIMDS * CLOCK_HZ) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, default=len(SIZES), help="how many of the sizes, smallest first")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fginn32.py needs a GPU")
    ctx = mods_amd.Context(0)
    rs = np.random.RandomState(3)
    out = []
    for n1, n2 in SIZES[:args.sizes]:
        pos2 = rs.uniform(0, 1000, (n2, 2))
        for dim in DIMS:
            if dim == 128:
                t = (rs.randint(0, 256, (n2, dim)) >> 2).astype(np.float32)
                q = (rs.randint(0, 256, (n1, dim)) >> 2).astype(np.float32)
                u1, u2 = torch.from_numpy(q.astype(np.uint8)).cuda(), torch.from_numpy(t.astype(np.uint8)).cuda()
            else:
                t = rs.randn(n2, dim).astype(np.float32)
                q = np.where(rs.rand(n1, 1) < 0.6, t[rs.randint(0, n2, n1)] + 0.3 * rs.randn(n1, dim), rs.randn(n1, dim)).astype(np.float32)
            tq, tt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
            torch.cuda.synchronize()

            def f32():
                ctx.profile(True)
                rec = ctx.match_fginn_f32_device(tq.data_ptr(), n1, tt.data_ptr(), n2, dim, pos2)
                return ctx.fginn32_last_ms(), len(rec)

            def int8():
                ctx.profile(True)
                rec = ctx.match_fginn_device(u1.data_ptr(), n1, u2.data_ptr(), n2, pos2)
                st = ctx.kernel_stats()
                return st["match_fginn"]["ms"], st["match_sweep1"]["ms"], len(rec)

            for _ in range(args.warmup):
                f32()
                if dim == 128:
                    int8()
            pack, search, fg, s1, nrec, nrec8 = [], [], [], [], 0, None
            for _ in range(args.reps):
                (p, s), nrec = f32()
                pack.append(p); search.append(s)
                if dim == 128:
                    a, b, nrec8 = int8()
                    fg.append(a); s1.append(b)
            ctx.profile(False)
            geo = mods_amd.fginn32_geometry(n1, n2, dim)
            med = float(np.median(search)) * 1e3
            bound = valu_bound_us(n1, n2, geo["DK"])
            row = {"n1": n1, "n2": n2, "dim": dim, "geometry": geo, "records": nrec, "repeats": args.reps,
                   "pack_us": float(np.median(pack)) * 1e3, "search_us": med, "search_min_us": float(np.min(search)) * 1e3,
                   "search_max_us": float(np.max(search)) * 1e3, "pairs_per_s": n1 * n2 / (med * 1e-6), "valu_bound_us": bound,
                   "bound_fraction": bound / med}
            if dim == 128:
                row.update({"int8_records": nrec8, "fginn_us": float(np.median(fg)) * 1e3, "sweep1_us": float(np.median(s1)) * 1e3})
            out.append(row)
    ctx.close()
    print(json.dumps({"bench": "fginn32", "rows": out}))


if __name__ == "__main__":
    main()
