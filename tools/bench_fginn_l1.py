#!/usr/bin/env python3
"""Timing of the L1 FGINN searches with HIP events: the f32 search with the L1 chain beside the L2 chain (kernels_fginn32.hip), and at
128 columns of integer rows the byte-row search (kernels_fginn_l1.hip) beside the f32-L1 search and the int8 L2 matcher.

Sizes 2 000 x 2 000, 8 192 x 8 192 and 24 123 x 23 632.  One process; per size and block --warmup (3) calls of every entry, then
--reps (21) repetitions in which the entries of a block ALTERNATE on the same rows, so that they share the machine's state.
  block a    dim 64 / 128 / 256, seeded Gaussian rows: f32-L1, f32-L2
  block b    128 columns holding the integers 0..255: u8-L1 (modsx_match_fginn_l1_device), f32-L1 and f32-L2 on the same rows widened
             to f32, and the int8 L2 matcher (modsx_match_fginn_device)
  measured   search_us: median [min, max] of the search launches (top-4 sweep + merge) between device events under modsx_profile;
             pack_us: the two packing launches; for the int8 matcher fginn_us (every launch of class match_fginn)
  computed   valu_bound_us = n1 n2 / 64 x VALU_PER_PAIR wave instructions x 2 cycles each / (256 CUs x 4 SIMDs x 2.4 GHz) and
             bound_fraction = valu_bound_us / search_us, as tools/bench_fginn32.py computes them.  VALU_PER_PAIR: the vector
             instructions per (query, train) of the sweep loop counted in the kernel's ISA, the key's insertion included
             (DESIGN.md 9.21).
Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mods_amd

SIZES = ((2000, 2000), (8192, 8192), (24123, 23632))
DIMS = (64, 128, 256)
VALU_PER_PAIR = {"l2": {64: 195, 128: 387, 256: 744}, "l1": {64: 179, 128: 307, 256: 606}, "u8": 57.5}
SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 256 * 4, 2.4e9, 2.0


def bound_us(n1, n2, valu):
    return n1 * n2 / 64.0 * valu * CYCLES_PER_VALU / (SIMDS * CLOCK_HZ) * 1e6


def stats(ms, n1, n2, valu):
    us = np.asarray(ms) * 1e3
    med = float(np.median(us))
    out = {"search_us": med, "search_min_us": float(us.min()), "search_max_us": float(us.max()), "pairs_per_s": n1 * n2 / (med * 1e-6)}
    if valu:
        out.update({"valu_per_pair": valu, "valu_bound_us": bound_us(n1, n2, valu), "bound_fraction": bound_us(n1, n2, valu) / med})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, default=len(SIZES), help="how many of the sizes, smallest first")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fginn_l1.py needs a GPU")
    ctx = mods_amd.Context(0)
    rs = np.random.RandomState(3)
    L1, L2 = mods_amd.DIST_L1, mods_amd.DIST_L2
    out = []

    def run(entries):
        """entries: name -> callable returning (search ms, pack ms, records); alternating repetitions"""
        for _ in range(args.warmup):
            for f in entries.values():
                f()
        got = {k: ([], [], 0) for k in entries}
        for _ in range(args.reps):
            for k, f in entries.items():
                s, p, n = f()
                got[k][0].append(s); got[k][1].append(p)
                got[k] = (got[k][0], got[k][1], n)
        return got

    for n1, n2 in SIZES[:args.sizes]:
        pos2 = rs.uniform(0, 1000, (n2, 2))
        for dim in DIMS:
            t = rs.randn(n2, dim).astype(np.float32)
            q = np.where(rs.rand(n1, 1) < 0.6, t[rs.randint(0, n2, n1)] + 0.3 * rs.randn(n1, dim), rs.randn(n1, dim)).astype(np.float32)
            tq, tt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
            torch.cuda.synchronize()

            def f32(dist, tq=tq, tt=tt, dim=dim):
                ctx.profile(True)
                rec = ctx.match_fginn_f32_device(tq.data_ptr(), n1, tt.data_ptr(), n2, dim, pos2, dist=dist)
                pack, search = ctx.fginn32_last_ms()
                return search, pack, len(rec)

            got = run({"f32_l1": lambda: f32(L1), "f32_l2": lambda: f32(L2)})
            row = {"block": "a", "n1": n1, "n2": n2, "dim": dim, "geometry": mods_amd.fginn32_geometry(n1, n2, dim), "repeats": args.reps}
            for k, kind in (("f32_l1", "l1"), ("f32_l2", "l2")):
                row[k] = dict(stats(got[k][0], n1, n2, VALU_PER_PAIR[kind][dim]), pack_us=float(np.median(got[k][1])) * 1e3, records=got[k][2])
            out.append(row)

        t = rs.randint(0, 256, (n2, 128)).astype(np.uint8)
        q = np.where(rs.rand(n1, 1) < 0.6, np.clip(t[rs.randint(0, n2, n1)].astype(np.int32) + rs.randint(-25, 26, (n1, 128)), 0, 255),
                     rs.randint(0, 256, (n1, 128))).astype(np.uint8)
        u1, u2 = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
        tq, tt = torch.from_numpy(q.astype(np.float32)).cuda(), torch.from_numpy(t.astype(np.float32)).cuda()
        torch.cuda.synchronize()

        def u8():
            ctx.profile(True)
            rec = ctx.match_fginn_l1_device(u1.data_ptr(), n1, u2.data_ptr(), n2, pos2)
            pack, search = ctx.fginn32_last_ms()
            return search, pack, len(rec)

        def f32i(dist):
            ctx.profile(True)
            rec = ctx.match_fginn_f32_device(tq.data_ptr(), n1, tt.data_ptr(), n2, 128, pos2, dist=dist)
            pack, search = ctx.fginn32_last_ms()
            return search, pack, len(rec)

        def int8():
            ctx.profile(True)
            rec = ctx.match_fginn_device(u1.data_ptr(), n1, u2.data_ptr(), n2, pos2)
            st = ctx.kernel_stats()
            return st["match_fginn"]["ms"], 0.0, len(rec)

        got = run({"u8_l1": u8, "f32_l1": lambda: f32i(L1), "f32_l2": lambda: f32i(L2), "int8_l2": int8})
        ctx.profile(False)
        row = {"block": "b", "n1": n1, "n2": n2, "dim": 128, "geometry_u8": mods_amd.fginn_l1_geometry(n1, n2),
               "geometry_f32": mods_amd.fginn32_geometry(n1, n2, 128), "repeats": args.reps}
        for k, valu in (("u8_l1", VALU_PER_PAIR["u8"]), ("f32_l1", VALU_PER_PAIR["l1"][128]), ("f32_l2", VALU_PER_PAIR["l2"][128]), ("int8_l2", None)):
            row[k] = dict(stats(got[k][0], n1, n2, valu), pack_us=float(np.median(got[k][1])) * 1e3, records=got[k][2])
        assert row["u8_l1"]["records"] == row["f32_l1"]["records"] and row["f32_l2"]["records"] == row["int8_l2"]["records"]
        row["u8_faster_than_f32_l1_ranges_apart"] = row["u8_l1"]["search_max_us"] < row["f32_l1"]["search_min_us"]
        out.append(row)
    ctx.close()
    print(json.dumps({"bench": "fginn_l1", "rows": out}))


if __name__ == "__main__":
    main()
