#!/usr/bin/env python3
"""Child process of tests/test_gpu_match_shapes.py:  match_shape_child.py IN.npz OUT.npz

MODSX_MATCH_QSETS and MODSX_SWEEP1_FAT are read once per process, so every forced shape of k_match_sweep1 gets a process of its own.
It opens ONE context, runs every case of IN through Context.match_fginn and writes the tentatives and, per call, what
mods_amd.last_match_geometry() reported; with `batch` set in IN it also runs the ten-pair mixed-size batch of
test_gpu_parity.test_grouped_pairs_equal_single_pairs (tests/common.grouped_pair_hosts around the pair in IN) through match_pairs and through match_pair, one by one, on that context.
Nothing is compared here: the parent holds the references.  Progress goes to stderr, one line per case, so that the tail of a
child that did not come back says where it was."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEO = ("qs", "fat", "S", "tiles_per_split", "ntiles_ub")
PAIR_SCALARS = ("n_tentatives", "n_verified", "ransac_samples")


def put_pair(out, key, r):
    out[key + "_regions"] = np.array(r["n_regions"])
    out[key + "_scalars"] = np.array([r[f] for f in PAIR_SCALARS])
    out[key + "_tentatives"] = r["tentatives"]
    out[key + "_verified"] = np.asarray(r["verified"])
    out[key + "_H"] = np.asarray(r["H"])


def main(inp, outp):
    import mods_amd
    z = np.load(inp)
    t0 = time.time()
    ctx = mods_amd.Context(0)
    out = {"t_context": np.array(time.time() - t0)}
    names = [str(n) for n in z["names"]]
    secs = []
    for i, name in enumerate(names):
        d1, d2 = z["d1_%d" % i].astype(np.float32), z["d2_%d" % i].astype(np.float32)
        pos2 = z["pos2_%d" % i]
        t1 = time.time()
        for j, (ratio, cd, nn) in enumerate(z["params_%d" % i]):
            print("case %s %r" % (name, (float(ratio), float(cd), int(nn))), file=sys.stderr, flush=True)
            out["tent_%d_%d" % (i, j)] = ctx.match_fginn(d1, d2, pos2, float(ratio), float(cd), int(nn))
            g = mods_amd.last_match_geometry()
            out["geo_%d_%d" % (i, j)] = np.array([g[k] for k in GEO])
        secs.append(time.time() - t1)
    out["case_seconds"] = np.array(secs)
    if int(z["batch"]):
        print("batch", file=sys.stderr, flush=True)
        from tests.common import grouped_pair_hosts
        dev = [(ctx.upload(x), ctx.upload(y)) for x, y in grouped_pair_hosts(z["pair_a"], z["pair_b"])]
        par = mods_amd.default_pair_params(ransac_seed=9)
        for i, (x, y) in enumerate(dev):
            put_pair(out, "single_%d" % i, ctx.match_pair(x, y, par))
        g = mods_amd.last_match_geometry()
        out["geo_single"] = np.array([g[k] for k in GEO])
        got = mods_amd.match_pairs([ctx], [x for x, _ in dev], [y for _, y in dev], par)
        g = mods_amd.last_match_geometry()
        out["geo_batch"] = np.array([g[k] for k in GEO])
        out["n_batch"] = np.array(len(got))
        for i, r in enumerate(got):
            put_pair(out, "batch_%d" % i, r)
        for x, y in dev:
            x.free(); y.free()
    ctx.close()
    out["t_total"] = np.array(time.time() - t0)
    np.savez(outp, **out)
    print("done", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
