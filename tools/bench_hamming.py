#!/usr/bin/env python3
"""Timing of the Hamming matcher's launches (kernels_hamming.hip) with HIP events, beside the L2 matcher on the same n1 x n2.

Sizes 2 000 x 2 000, 8 192 x 8 192 and 24 123 x 23 632 (the size of profiles/r06_match_m24k.txt), widths 32 and 64 bytes.  Per
size and width: --warmup calls, then --reps (>= 20) timed repetitions that ALTERNATE modsx_match_hamming_device with
modsx_match_fginn_device on the same n1, n2 in this process, so the two share the machine's state; medians are reported.
  measured   pack_us (the two k_hamming_pack launches), search_us (k_hamming_2nn + k_hamming_merge), fginn_us (every launch of the
             L2 matcher, class match_fginn) and sweep1_us (its contraction launch alone) -- device events under modsx_profile
  computed   pairs_per_s = n1 n2 / search time; valu_bound_us = n1 n2 / 64 x (2 WK + 3.75) wave instructions (WK v_xor, WK v_bcnt,
             v_lshl_or, v_max, v_min, half a v_min3 and a quarter of the LDS address move per pair -- counted in the kernel's
             ISA) x 2 cycles each / (256 CUs x 4 SIMDs x 2.4 GHz); bound_fraction = valu_bound_us / search_us
The rows are seeded random bytes (queries: noisy copies of trains).  Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mods_amd

SIZES = ((2000, 2000), (8192, 8192), (24123, 23632))
WIDTHS = (32, 64)
SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 256 * 4, 2.4e9, 2.0


def kernel_width(nbytes):
    W = (nbytes + 3) // 4
    return 1 if W <= 1 else 2 if W <= 2 else 4 if W <= 4 else 8 if W <= 8 else 16


def valu_bound_us(n1, n2, nbytes):
    per_pair = 2 * kernel_width(nbytes) + 3.75
    return n1 * n2 / 64.0 * per_pair * CYCLES_PER_VALU / (SIMDS * CLOCK_HZ) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=60.0)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_hamming.py needs a GPU")
    ctx = mods_amd.Context(0)
    rs = np.random.RandomState(3)
    out = []
    for n1, n2 in SIZES:
        sift1 = torch.from_numpy(rs.randint(0, 256, (n1, 128)).astype(np.uint8) >> 2).cuda()
        sift2 = torch.from_numpy(rs.randint(0, 256, (n2, 128)).astype(np.uint8) >> 2).cuda()
        pos2 = rs.uniform(0, 1000, (n2, 2))
        for nbytes in WIDTHS:
            t = rs.randint(0, 256, (n2, nbytes)).astype(np.uint8)
            q = t[rs.randint(0, n2, n1)] ^ np.packbits(rs.rand(n1, 8 * nbytes) < rs.uniform(0, 0.5, (n1, 1)), axis=1)
            tq, tt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
            torch.cuda.synchronize()

            def ham():
                ctx.profile(True)
                rec = ctx.match_hamming_device(tq.data_ptr(), n1, tt.data_ptr(), n2, nbytes, args.threshold)
                return ctx.hamming_last_ms(), len(rec)

            def fginn():
                ctx.profile(True)
                ctx.match_fginn_device(sift1.data_ptr(), n1, sift2.data_ptr(), n2, pos2)
                st = ctx.kernel_stats()
                return st["match_fginn"]["ms"], st["match_sweep1"]["ms"]

            for _ in range(args.warmup):
                ham(); fginn()
            pack, search, fg, s1, nrec = [], [], [], [], 0
            for _ in range(args.reps):
                (p, s), nrec = ham()
                a, b = fginn()
                pack.append(p); search.append(s); fg.append(a); s1.append(b)
            ctx.profile(False)
            geo = mods_amd.hamming_geometry(n1, n2, nbytes)
            med = float(np.median(search)) * 1e3
            bound = valu_bound_us(n1, n2, nbytes)
            out.append({"n1": n1, "n2": n2, "nbytes": nbytes, "geometry": geo, "records": nrec, "repeats": args.reps,
                        "pack_us": float(np.median(pack)) * 1e3, "search_us": med, "search_min_us": float(np.min(search)) * 1e3,
                        "search_max_us": float(np.max(search)) * 1e3, "pairs_per_s": n1 * n2 / (med * 1e-6),
                        "valu_bound_us": bound, "bound_fraction": bound / med,
                        "fginn_us": float(np.median(fg)) * 1e3, "sweep1_us": float(np.median(s1)) * 1e3})
    ctx.close()
    print(json.dumps({"bench": "hamming", "results": out}))


if __name__ == "__main__":
    main()
