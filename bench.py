#!/usr/bin/env python3
"""Benchmark of the MODS hot path on MI355X (BASELINE.json: image-pairs/s + descriptors matched/s, 1024x768, HessAff+SIFT).

A step = one pass of the path over one batch of 64 synthetic 1024x768 image pairs per GPU (16 contexts take the pairs of a
step from a shared counter): per image the affine view ladder
(default TiltSet 1,2,4,6,8 at Phi 120 = 31 views, synth-detection.cpp:103-234) -> Hessian-Affine + Baumberg -> dominant
orientation -> RootSIFT per view, then brute-force FGINN matching of the ~24 k x 24 k descriptors on the int8 matrix cores
(matching.cpp:357-461), duplicate filtering and LO-RANSAC (H).  All images are resident in HBM before the timed region.

  --config views31 (default) | views61 | views11 | views8 | views1 | wxbs      workload of the JSON line
  --config ladder    configs[3] on one GPU: every MSER and HessianAffine step of build/iters_mods_cviu.ini (27 MSER + 61
             HessianAffine views per image, minMatches forced high so that all steps run), with the MSER host share
  --gpus N   one process per GPU (torch.distributed.run).  --shard pairs (default): independent pairs per rank, no
             collective; with N > 1 the same line carries `scaling_views`, the north-star's view-parallel mode measured
             right after: every pair's views are split over the N ranks (view v -> rank v mod N), the region rows + u8
             descriptors are all-gathered over RCCL/xGMI inside the library (modsx_detect_describe_views_sharded) and the
             query rows of the match are split over the ranks; the batch grows with N (weak scaling: per-GPU work fixed).
             --shard views makes that mode the headline value instead.
  --loopback W   one GPU: the view-sharded path with W in-process ranks (loopback transport: the all-gather is W
             device-to-device copies, everything else is the code the RCCL transport runs), workers / W lanes per rank
  --full     also run the legs beyond the headline (a plain run sets up, warms up, times the K steps and prints the line):
             the per-step-barrier form, the upload form, configs[4]'s F verification, the ladder's parts and latencies, the
             per-kernel and roofline legs, the short runs under `extra` (--no-extra), the CPU baseline and parity (--no-cpu-baseline)
  --dump-outputs DIR   after the timed steps, write what the last timed step computed (rank 0's pairs) as DIR/<name>.npy
Rank 0 prints ONE JSON line: value = pairs/s of the whole job, ms_per_step = milliseconds of one timed step.  With --full also
`roofline` = the distance kernels (all k_match_* launches -- pack, sweep 1, decide, resolve -- on the descriptors of this run)
against the int8 MFMA peak, `roofline_describe` = the describe stage against HBM with SURVEY section 8(d) bytes, `cpu_baseline` =
the CPU oracle (restatement of the reference's CPU path) on the same workload with all host cores and with one, `parity` = GPU vs
that CPU path on one pair of the run.
"""
import argparse
import itertools
import subprocess
import tempfile
import threading
import json
import os
import sys
import time
import resource

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# keep the host tables of a pair mapped between calls (modsx.h: opt-in, it changes malloc for the whole process -- this one is ours)
os.environ.setdefault("MODSX_MALLOC_TUNE", "1")

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
INT8_PEAK_TOPS = 5000.0      # dense int8 matrix peak (~2x the 2.5 PF bf16 dense peak)
CONFIGS = {   # name -> (tilts, phi, detector mode, description)
    "views1": ("1", 360.0, "configs[1]: 1 view"),
    "views8": ("1,2,3,4,6", 360.0, "configs[2]: 8 affine-synth views (TiltSet 1,2,3,4,6, Phi 360)"),
    "views11": ("1,2,4,6,8", 360.0, "11 views (TiltSet 1,2,4,6,8, Phi 360: iters_mods_cviu.ini HessianAffine step)"),
    "views31": ("1,2,4,6,8", 120.0, "31 views (TiltSet 1,2,4,6,8, Phi 120)"),
    "views61": ("1,2,4,6,8", 60.0, "61 views (TiltSet 1,2,4,6,8, Phi 60)"),
    # configs[4]: 1920x1080 pairs with the parameter set of config_iter_mods_cviu_wxbs.ini (NotLessThanRegions 2000, maxAngles 5
    # on the 5.1962 region with the Half-folded orientation histogram, the RootSIFT and HalfRootSIFT classes of every WxBS step,
    # contradDist 10, duplicateDist 3, err_threshold 4, max_samples 1e6), H then F
    "wxbs": ("1", 360.0, "configs[4]: WxBS parameter set (RootSIFT + HalfRootSIFT classes), identity view"),
    "ladder": ("1,2,4,6,8", 60.0, "configs[3]: iters_mods_cviu.ini, all MSER + HessianAffine steps (27 + 61 views per image)"),
}
# [MSER2], [MSER3], [HessianAffine4..6] of build/iters_mods_cviu.ini: detector, ScaleSet, TiltSet, Phi, initSigma, FGINN ratio
CVIU_LADDER = ((3, [1, 0.25, 0.125], [1], 360.0, 0.8, 0.85), (3, [1, 0.25, 0.125], [1, 3, 6, 9], 360.0, 0.8, 0.8),
               (0, [1], [1, 2, 4, 6, 8], 360.0, 0.2, 0.8), (0, [1], [1, 2, 4, 6, 8], 120.0, 0.2, 0.8),
               (0, [1], [1, 2, 4, 6, 8], 60.0, 0.2, 0.8))


def cviu_ladder_steps(M, only=None):
    prev, steps = {0: [], 3: []}, []
    for det, scales, tilts, phi, sigma, ratio in CVIU_LADDER:
        v = M.set_vs_pars(scales, tilts, phi, sigma, 1, prev[det])
        if v and (only is None or det == only):
            steps.append((v, ratio, det))
    return steps
# config_iter_mods_cviu_wxbs.ini + the step structure of iters_mods_cviu_wxbs.ini [HessianAffine4] (:56-62): Descriptors=RootSIFT,
# HalfRootSIFT, FGINNThreshold=0.8,0.8 -- one Half-folded orientation pass, both descriptors, two classes matched separately
WXBS = dict(mode=4, threshold=5.3333, reg_number=2000, ori_mrSize=5.1962, ori_maxAngles=5, ori_threshold=0.8, desc_mrSize=5.1962,
            desc_photoNorm=1, desc_maxBinValue=0.2, descs=[(1, 0.8), (3, 0.8)], contradDist=10.0, duplicateDist=3.0,
            err_threshold=4.0, confidence=0.99, max_samples=1000000, localOptimization=1, LAFCoef=3.0, HLAFCoef=13.0, doSymmCheck=1)


def cpu_info():
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    # a container's CPU allowance (cgroup v2 cpu.max / v1 cfs quota): the GPU boxes show 256 logical CPUs and allow 16 --
    # more runnable threads than that only buy throttling, so the CPU baseline uses (and reports) the allowance
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota:
        usable = max(1, min(usable, int(quota + 0.5)))
    return model, os.cpu_count() or 1, usable


def oracle_pair_views(O, a, b, views_o, params, threads, seed=1, query_cap=None, one_image=False):
    """The CPU path (oracle = restatement of the reference) for one pair under a view ladder.  Parallel structure of the
    reference: images x views in parallel (mods.cpp:255-271, imagerepresentation.cpp:612-622), here a thread pool over
    (image, view) tasks (ctypes releases the GIL) + OpenMP over the query rows of the brute-force kNN."""
    import numpy as np
    import ctypes
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from common import laf_of
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(int(threads))
    except OSError:
        pass
    t0 = time.time()
    imgs = [a] if one_image else [a, b]

    def one(task):
        im, v = task
        return O.detect_describe_views(imgs[im], [views_o[v]])
    tasks = [(i, v) for i in range(len(imgs)) for v in range(len(views_o))]
    if threads > 1:
        with ThreadPoolExecutor(threads) as pool:
            parts = list(pool.map(one, tasks))
    else:
        parts = [one(t) for t in tasks]
    regs, desc = [], []
    for i in range(len(imgs)):
        rs, ds, size = [], [], 0
        for v in range(len(views_o)):
            r, d = parts[i * len(views_o) + v]
            r = r.copy()
            if v and len(r):      # the per-view call numbered its block from 0 and cannot know the view index
                ident = abs(views_o[v].tilt - 1) <= 0.1 and abs(views_o[v].phi) <= 0.2 and abs(views_o[v].zoom - 1) <= 0.1
                r["img_id"] = 0 if ident else v
            r["id"] += size; r["parent_id"] += size
            size += len(r)
            rs.append(r); ds.append(d)
        regs.append(np.concatenate(rs)); desc.append(np.concatenate(ds))
    t1 = time.time()
    out = dict(t_extract=t1 - t0, regs=regs, desc=desc)
    if one_image:
        return out
    r1, r2, d1, d2 = regs[0], regs[1], desc[0], desc[1]
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    nq = len(d1) if query_cap is None else min(query_cap, len(d1))
    tent = O.match_fginn(d1[:nq], d2, pos2, params.match_ratio, params.contradDist)
    t2 = time.time()
    out.update(t_match=t2 - t1, n_match_queries=nq, tent=tent)
    if query_cap is not None and nq < len(d1):
        return out
    pts = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                    r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = O.duplicate_filtering(pts, tent["ratio"], params.duplicateDist, True)
    sel = order[keep]
    tu, pu = tent[sel], pts[sel]
    res = None
    if O.ref_available():
        res = O.loransac_h(pu, laf_of(r1, tu["q"]), laf_of(r2, tu["t0"]), err_threshold=params.err_threshold,
                           confidence=params.confidence, max_samples=params.max_samples, seed=seed)
    t3 = time.time()
    out.update(t_verify=t3 - t2, uniq=tu, pts=pu, ransac=res, total=t3 - t0, laf1=laf_of(r1, tu["q"]), laf2=laf_of(r2, tu["t0"]))
    return out


DUMP_BYTES_MAX = 60 << 20     # --dump-outputs: all files together stay below 64 MB


def dump_outputs(path, results):
    """--dump-outputs: the per-pair results of the last timed step, as a caller of the path receives them (None = a pair another rank
    verified), one .npy per array, rows in the step's pair order:
      pair_index [P]  counts [P, 8] (regions 1, regions 2, tentatives, unique, RANSAC inliers, verified, RANSAC samples, LO count)
      H [P, 3, 3]     tentative_ids [T, 4] (q, t0, tj, t1)   tentative_dist [T, 4] (d1, d2, d2by2ndcl, ratio)
      tentative_pair [T] (its pair)   ransac_inlier [T], verified [T] (0 / 1)   tentative_rows [T] (its row in the full list)
    The unique tentatives of all pairs are one list; past DUMP_BYTES_MAX a fixed, seeded sample of its rows is written.  Integers
    travel as float32 while they are exact there (below 2^24), as float64 otherwise; distances and H as float64."""
    import numpy as np

    def exact(x):
        x = np.asarray(x)
        return x.astype(np.float32) if x.size == 0 or np.abs(x).max() < (1 << 24) else x.astype(np.float64)
    idx = [i for i, r in enumerate(results) if r is not None]
    rs = [results[i] for i in idx]
    counts = np.array([[r["n_regions"][0], r["n_regions"][1], r["n_tentatives"], r["n_unique"], r["n_ransac_inliers"],
                        r["n_verified"], r["ransac_samples"], r["ransac_lo"]] for r in rs], np.float64).reshape(-1, 8)
    H = np.array([np.asarray(r["H"], np.float64).reshape(3, 3) for r in rs]).reshape(-1, 3, 3)
    tents = [r["tentatives"] for r in rs]
    t = np.concatenate(tents) if tents else np.zeros(0)
    pair = np.concatenate([np.full(len(x), i, np.int64) for i, x in zip(idx, tents)]) if tents else np.zeros(0, np.int64)
    inl = np.concatenate([r["ransac_inlier"] for r in rs]) if rs else np.zeros(0, bool)
    ver = np.concatenate([r["verified"] for r in rs]) if rs else np.zeros(0, bool)
    rows = np.arange(len(t))
    row_bytes = 64 if len(t) < (1 << 24) and (not len(counts) or counts[:, :2].max() < (1 << 24)) else 88
    cap = max(0, (DUMP_BYTES_MAX - counts.nbytes - H.nbytes - 8 * len(idx)) // row_bytes)
    if len(t) > cap:
        rows = np.sort(np.random.RandomState(20260).choice(len(t), cap, replace=False))
    t = t[rows]
    arrays = {
        "pair_index": np.asarray(idx, np.float64), "counts": counts, "H": H,
        "tentative_ids": exact(np.stack([t[f] for f in ("q", "t0", "tj", "t1")], 1).reshape(-1, 4) if len(t) else np.zeros((0, 4))),
        "tentative_dist": (np.stack([t[f] for f in ("d1", "d2", "d2by2ndcl", "ratio")], 1).reshape(-1, 4) if len(t)
                           else np.zeros((0, 4))).astype(np.float64),
        "tentative_pair": exact(pair[rows]), "ransac_inlier": inl[rows].astype(np.float32), "verified": ver[rows].astype(np.float32),
        "tentative_rows": exact(rows),
    }
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


class ShardGroup:
    """The view-sharded mode of a step.  RCCL: this process is one rank, its contexts are the lanes of ONE communicator.
    Loopback (one GPU): W in-process ranks, each with its own contexts / lanes.  Pair i of a step runs on lane i % lanes of
    EVERY rank (static map: all ranks must issue the collectives of a lane in the same order); rank i % world verifies."""

    def __init__(self, mods_amd, device, lanes, dist=None, loopback=0, ctxs=None, exchange="allgather"):
        from mods_amd import distributed as D
        self.lanes = lanes
        self.exchange = exchange
        if loopback:
            self.world = loopback
            uid = mods_amd.comm_loopback_id(loopback)
            self.ctxs = [[mods_amd.Context(device) for _ in range(lanes)] for _ in range(loopback)]
            self.comms = [D.NativeComm(self.ctxs[r], rank=r, world=loopback, uid=uid) for r in range(loopback)]
            self.own_ctxs = True
        else:
            self.world = dist.get_world_size() if dist is not None else 1
            self.ctxs = [list(ctxs[:lanes])]
            self.comms = [D.NativeComm(self.ctxs[0], dist)]
            self.own_ctxs = False
        if exchange == "owner":        # a pair's rows travel to the rank that matches and verifies it, not to every rank
            for cm in self.comms:
                cm.set_exchange(mods_amd.EXCHANGE_OWNER)
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(len(self.comms) * lanes)

    def step(self, i1, i2, views, params):
        """Chunks of k = world consecutive pairs go through ONE sharded call each (modsx_match_pairs_views_sharded: one exchange for
        the 2 k image sides, one result all-gather): a rank's launch sets hold ~2 * 31 views whatever the world size, and the
        collectives per pair fall with it.  Chunk j runs on lane j % lanes of every rank; pair g is verified by rank g % world."""
        for cm in self.comms:
            cm.reset_lanes()
        k = max(1, min(8, self.world))
        chunks = [(c0, min(len(i1), c0 + k)) for c0 in range(0, len(i1), k)]

        def work(job):
            r, w = job
            cm = self.comms[r]
            out = []
            try:
                for j in range(w, len(chunks), self.lanes):
                    c0, c1 = chunks[j]
                    res = cm.match_pairs_views_sharded(w, i1[c0:c1], i2[c0:c1], views, params, owner_base=c0 % self.world, arrays=False)
                    for g, rr in enumerate(res):
                        if (c0 + g) % self.world == cm.rank:
                            out.append((c0 + g, rr))
            finally:
                cm.lane_done(w)
            return out
        res = [None] * len(i1)
        for part in self.pool.map(work, [(r, w) for r in range(len(self.comms)) for w in range(self.lanes)]):
            for i, r in part:
                if r is not None:
                    res[i] = r
        return res

    def synchronize(self):
        for cs in self.ctxs:
            for c in cs:
                c.synchronize()

    def describe(self):
        d = self.comms[0].describe()
        d["ranks_in_this_process"] = len(self.comms)
        d["exchange"] = self.exchange
        return d

    def close(self):
        self.pool.shutdown()
        for cm in self.comms:
            cm.close()
        if self.own_ctxs:
            for cs in self.ctxs:
                for c in cs:
                    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--step-barrier", action="store_true", help="a host-side barrier after every timed step (the form of rounds 1-4)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=768)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--config", type=str, default="views31", choices=sorted(CONFIGS))
    ap.add_argument("--tilts", type=str, default="", help="override the tilt set of --config, e.g. 1,2,3,4,6")
    ap.add_argument("--phi", type=float, default=0.0)
    ap.add_argument("--batch", type=int, default=0, help="pairs per step per GPU (default 64; 256 for views1, 128 for wxbs)")
    ap.add_argument("--blobs", type=int, default=0, help="blobs per 1024x768 of the synthetic scene (0 = per config)")
    ap.add_argument("--workers", type=int, default=16, help="contexts (thread + stream) per GPU")
    ap.add_argument("--distinct", type=int, default=0, help="distinct synthetic pairs cycled through the batch (0 = as many as a step holds: "
                    "every pair of a step is another pair, as BASELINE.json's configs state them)")
    ap.add_argument("--init-sigma", type=float, default=0.2)
    ap.add_argument("--shard", type=str, default="", choices=["", "pairs", "views"])
    ap.add_argument("--loopback", type=int, default=0, help="one GPU: W in-process ranks of the view-sharded path")
    ap.add_argument("--exchange", type=str, default="allgather", choices=["allgather", "owner"],
                    help="view-sharded path: rows of a pair to every rank (the north star's all-gather) or to its owner rank only")
    ap.add_argument("--no-scaling-views", action="store_true", help="N > 1: skip the view-sharded second measurement")
    ap.add_argument("--batch-api", action="store_true", help="multi-view configs: run a step as ONE modsx_match_pairs_views call")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the short 1/8/11-view and 4000-blob runs reported under `extra`")
    ap.add_argument("--full", action="store_true", help="also the legs beyond the headline: step-barrier and upload forms, wxbs F, ladder "
                    "parts, per-kernel and roofline legs, `extra`, CPU baseline and parity (default: the headline alone)")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="write the results of the last timed step (rank 0's pairs) as DIR/<name>.npy (float32 / float64, <= 64 MB)")
    args = ap.parse_args()

    import numpy as np
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    exit_code = 0
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    # headline: pairs over ranks (no collective: independent pairs are the reference's batch use); the north star's
    # view-parallel mode is measured in the same run when N > 1 (`scaling_views`), or as the headline with --shard views
    shard = args.shard or "pairs"
    if args.loopback:
        if world > 1:
            raise SystemExit("--loopback is a one-process mode")
        shard = "views"

    import mods_amd
    from mods_amd import synthetic
    tilts, phi, cfg_desc = CONFIGS[args.config]
    wxbs = args.config == "wxbs"
    ladder = args.config == "ladder"
    if wxbs:
        args.rows, args.cols = 1080, 1920
    if args.tilts:
        tilts, phi = args.tilts, (args.phi or 360.0)
        cfg_desc = "tilts %s, phi %g" % (tilts, phi)
    single_view = tilts == "1"
    # a step ends with the verification of its last pairs while the GPU drains: configs[1] (45 ms per 64 pairs) and
    # configs[4] take longer steps so that this tail stays a few per cent of the step
    batch = args.batch or (256 if (wxbs or single_view) else 64)   # configs[4]: "batch of 256 random 1920x1080 pairs"   # (the ladder ran 32 per step until round 4: two pairs per context and step, i.e. the step's tail with most contexts idle was 8 % of it: 46.9 against 51.0 pairs/s)
    # blob density of the synthetic scene: 4000 per 1024x768 for configs[1], [3], [4]; 5500 for
    # the multi-view headline so that the 31-view default carries the >= 50 k descriptors per pair the north star is quoted
    # on (the 4000-blob figure of the same configuration is reported under `extra`)
    blobs = args.blobs or (4000 if (single_view or wxbs or ladder) else 5500)
    nblobs = int(blobs * args.rows * args.cols / (768.0 * 1024))
    ctxs = [mods_amd.Context(local_rank) for _ in range(max(1, args.workers))]
    ctx = ctxs[0]
    pkw = dict(WXBS) if wxbs else dict(ori_mrSize=5.1962) if ladder else {}
    params = mods_amd.default_pair_params(ransac_seed=1, **pkw)
    views = mods_amd.set_vs_pars([1.0], [float(t) for t in tilts.split(",")], phi, args.init_sigma, 1, [])
    lsteps = cviu_ladder_steps(mods_amd) if ladder else None

    gen_procs = max(1, min(32, cpu_info()[2]))

    def make_images(seed0, count, nb, keep_host=True):
        """count distinct pairs: rendered by worker processes into a cache of u8 files (mods_amd/synthetic.py make_pairs), uploaded as
        f32.  configs[4] takes SURVEY section 8(d) item 5's seeds (1000 + i for image A, 2000 + i for B's noise), the other
        configurations the seeds of rounds 1-5 (seed0 + 17 i, B: + 42000)."""
        count = max(1, count)
        if wxbs:
            specs = [(args.rows, args.cols, nb, 1000 + i, 2000 + i) for i in range(count)]
        else:
            specs = [(args.rows, args.cols, nb, seed0 + 17 * i, seed0 + 17 * i + 42000) for i in range(count)]
        host = synthetic.make_pairs(specs, procs=gen_procs, as_u8=True)
        devp = [(ctx.upload(a), ctx.upload(b)) for a, b, _ in host]       # u8 in, f32 on the device (modsx_image_upload)
        return host, devp

    # pairs: in the view-sharded mode every rank holds every pair of the (N x larger) batch; otherwise its own pairs
    views_world = args.loopback or world
    if shard == "views":
        seed0, nbatch = 12345, batch * views_world
    else:
        seed0, nbatch = 12345 + 1000 * rank, batch
    t_gen = time.perf_counter()
    distinct = args.distinct or nbatch
    pairs_host, dev = make_images(seed0, distinct, nblobs)
    t_gen = time.perf_counter() - t_gen
    Hgt = pairs_host[0][2]
    imgs1 = [dev[i % len(dev)][0] for i in range(nbatch)]
    imgs2 = [dev[i % len(dev)][1] for i in range(nbatch)]

    group = None
    if shard == "views":
        lanes = max(1, len(ctxs) // args.loopback) if args.loopback else len(ctxs)
        group = ShardGroup(mods_amd, local_rank, lanes, dist=dist, loopback=args.loopback, ctxs=ctxs, exchange=args.exchange)

    def barrier(g=None):
        for c in ctxs:
            c.synchronize()
        if g is not None:
            g.synchronize()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(len(ctxs))

    def run_batch(vw=views, single=single_view, i1=imgs1, i2=imgs2, cx=ctxs, g=group, steps_l=lsteps):
        if g is not None:
            return g.step(i1, i2, vw, params)
        if single:
            return mods_amd.match_pairs(cx, i1, i2, params)
        if args.batch_api and steps_l is None:
            # the library's own batch loop (modsx_match_pairs_views): 4-5 % below the persistent python threads of the default
            # path, whose threads are not re-created per step
            return mods_amd.match_pairs_views(cx, i1, i2, vw, params, arrays=False)

        # multi-view pairs: one python thread per context (ctypes releases the GIL inside the library).  The contexts take the
        # pairs of the step from a shared counter, so that the step ends at most one pair after its last pair was started
        # (with a static pair -> context map the step waited for the context with the most expensive pairs: 15 % of the
        # GPU's time was idle at step boundaries).
        nxt = itertools.count()
        lock = threading.Lock()

        def work(w):
            out = []
            while True:
                with lock:
                    i = next(nxt)
                if i >= len(i1):
                    return out
                if steps_l is not None:
                    out.append((i, cx[w].match_ladder(i1[i], i2[i], steps_l, params, min_matches=10 ** 6)[0]))
                else:
                    out.append((i, cx[w].match_pair_views(i1[i], i2[i], vw, params)))
        res = [None] * len(i1)
        for part in pool.map(work, range(len(cx))):
            for i, r in part:
                res[i] = r
        return res

    host_cpu = {}

    def run_steps_back_to_back(nsteps, i1=imgs1, i2=imgs2, cx=ctxs):
        """K steps of the default (multi-view, pair-sharded) workload issued back to back: every context goes from the last
        pair of step k straight to the first of step k + 1, as a training loop issues its steps without a host-side barrier
        between them.  The work is that of K calls of run_batch; what goes away is the idle tail of each step (the last pairs
        finishing while most contexts wait for the step's barrier).  Returns the K steps' result lists."""
        n = len(i1)
        nxt = itertools.count()
        lock = threading.Lock()

        def work(w):
            out = []
            tc0 = time.thread_time()
            while True:
                with lock:
                    k = next(nxt)
                if k >= nsteps * n:
                    with lock:       # CPU of the contexts' own threads (the rest of the process' CPU: helper, pool and runtime threads)
                        host_cpu["ctx_threads"] = host_cpu.get("ctx_threads", 0.0) + time.thread_time() - tc0
                    return out
                out.append((k, cx[w].match_pair_views(i1[k % n], i2[k % n], views, params)))
        res = [[None] * n for _ in range(nsteps)]
        for part in pool.map(work, range(len(cx))):
            for k, r in part:
                res[k // n][k % n] = r
        return res

    def timed(run, warmup, steps, g=None, back_to_back=False):
        results = None
        for _ in range(warmup):
            results = run()
        barrier(g)
        sampler = os.environ.get("MODSX_HOST_SAMPLER") if not host_cpu.get("sampled") else None
        if sampler:      # tools/host_sampler.py: the library's sampling profiler over the first timed region (the headline's K steps)
            import ctypes as _C
            mods_amd.lib().modsx_debug_sampler.argtypes = [_C.c_int, _C.c_char_p, _C.c_int]
            mods_amd.lib().modsx_debug_sampler(1, None, 1000)
        ru0 = resource.getrusage(resource.RUSAGE_SELF)
        host_cpu["ctx_threads"] = 0.0
        t0 = time.perf_counter()
        nd = 0
        for results in (run_steps_back_to_back(steps) if back_to_back else (run() for _ in range(steps))):
            for r in results:
                if r is not None:
                    nd += r["n_regions"][0] + r["n_regions"][1]
        barrier(g)
        dt = time.perf_counter() - t0
        ru1 = resource.getrusage(resource.RUSAGE_SELF)
        if sampler:
            mods_amd.lib().modsx_debug_sampler(0, sampler.encode(), 0)
            host_cpu["sampled"] = True
        host_cpu["s"] = (ru1.ru_utime - ru0.ru_utime) + (ru1.ru_stime - ru0.ru_stime)     # this rank's threads, user + system
        host_cpu["sys"] = ru1.ru_stime - ru0.ru_stime
        host_cpu["ctx"] = host_cpu.get("ctx_threads", 0.0)
        return dt, nd, results

    def reduce_over_ranks(elapsed, nd):
        if dist is None:
            return elapsed, float(nd)
        t = torch.tensor([elapsed, float(nd)], device="cuda", dtype=torch.float64)
        tmax, tsum = t.clone(), t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        return float(tmax[0]), float(tsum[1])

    # the K timed steps are bracketed by a barrier + synchronize on both sides; the default workload issues them back to back
    # (--step-barrier: a host-side barrier after every step, the form of rounds 1-4, whose figure stays in the line beside it)
    b2b = group is None and not single_view and not args.batch_api and lsteps is None and not args.step_barrier
    elapsed, ndesc, results = timed(run_batch, args.warmup, args.steps, group, back_to_back=b2b)
    host_cpu_headline = host_cpu["s"]       # of the K timed steps (later legs run through timed() too)
    host_cpu_split = (host_cpu.get("ctx", 0.0), host_cpu.get("sys", 0.0))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, results)
    barrier_form = None
    if b2b and args.full:
        eb, nb_, _ = timed(run_batch, 0, args.steps, group)
        eb, nb_ = reduce_over_ranks(eb, nb_)
        barrier_form = {"value": args.steps * world * nbatch / eb, "unit": "image-pairs/s", "ms_per_step": 1e3 * eb / args.steps,
                        "note": "the same K steps with a host-side barrier after every step (rounds 1-4 reported this form)"}
    res = next((r for r in results if r is not None), None)
    verify_timed = mods_amd.last_batch_verify() if single_view else None   # host share of the last batch of the timed region
    verify_each_h = mods_amd.last_batch_verify_each() if single_view else None   # per pair, last step of the timed region

    # ---- the same steps with every pair's images handed over as HOST buffers (the reference loads a pair per iteration, mods.cpp:117-127):
    # `value` is measured with the images resident in HBM; this is the PCIe-inclusive figure beside it.  u8 grey images, as cv::imread
    # delivers them: modsx_image_update refills the two images a context keeps (no allocation per pair), the device converts to f32.
    upload_form = None
    if args.full and rank == 0 and group is None and lsteps is None and not os.environ.get("MODSX_BENCH_NO_UPLOAD_LEG"):
        nst = max(1, min(args.steps, 3))
        n = len(imgs1)
        hostA = [pairs_host[i % len(pairs_host)][0] for i in range(n)]
        hostB = [pairs_host[i % len(pairs_host)][1] for i in range(n)]
        up_s = [0.0]
        if single_view:
            # the batch API takes device images: the step's pairs are uploaded (one allocation + copy each), matched, freed
            barrier(group)
            tu0 = time.perf_counter()
            for _ in range(nst):
                tu = time.perf_counter()
                d1 = [ctx.upload(a_) for a_ in hostA]
                d2 = [ctx.upload(b_) for b_ in hostB]
                up_s[0] += time.perf_counter() - tu
                mods_amd.match_pairs(ctxs, d1, d2, params)
                for im_ in d1 + d2:
                    im_.free()
            barrier(group)
            du = time.perf_counter() - tu0
            note = "every step uploads its pairs (modsx_image_upload: allocation + H2D + conversion, one stream), then matches them: the upload is not overlapped"
        else:
            slots = [(c.upload(hostA[0]), c.upload(hostB[0])) for c in ctxs]
            nxt = itertools.count()
            lock = threading.Lock()

            def work_up(w):
                t_up = 0.0
                sa, sb = slots[w]
                while True:
                    with lock:
                        k = next(nxt)
                    if k >= nst * n:
                        return t_up
                    tu = time.perf_counter()
                    sa.update(hostA[k % n]); sb.update(hostB[k % n])
                    t_up += time.perf_counter() - tu
                    ctxs[w].match_pair_views(sa, sb, views, params)
            barrier(group)
            tu0 = time.perf_counter()
            up_s[0] = sum(pool.map(work_up, range(len(ctxs))))
            barrier(group)
            du = time.perf_counter() - tu0
            for sa, sb in slots:
                sa.free(); sb.free()
            note = ("every context refills its two images from host buffers before each pair (modsx_image_update on its own stream: H2D + "
                    "conversion, overlapped with the other contexts' kernels)")
        upload_form = {"value": nst * n / du, "unit": "image-pairs/s", "steps": nst, "upload_ms_per_pair": 1e3 * up_s[0] / (nst * n),
                       "bytes_per_pair": int(hostA[0].nbytes + hostB[0].nbytes), "note": note}
    wxbs_f = None
    if args.full and wxbs and rank == 0 and group is None:
        # configs[4] with epipolar verification: measured HERE, before any leg that brackets launches with timing events -- once a
        # context has recorded such events the runtime keeps per-dispatch completion signals on its queue, which costs the context's
        # host thread ~20 ms of CPU per pair from then on (tools/wxbs_cpu_probe.py: 8.5 -> 29 ms), and this leg is the one that is
        # short of CPU (rounds 3-5 measured it after the profiling legs: 245-285 pairs/s for what is 313-319)
        pF = mods_amd.default_pair_params(ransac_seed=1, useF=1, **WXBS)
        mods_amd.match_pairs(ctxs, imgs1, imgs2, pF)
        mods_amd.verify_device_stats(reset=True)
        ruF0 = resource.getrusage(resource.RUSAGE_SELF)
        ta = time.perf_counter()
        stF = 3
        # the stF steps' pairs in ONE call of the batch API (what back-to-back steps are for the per-pair calls: no idle tail of
        # 16 contexts and their verification helpers between steps); the per-step form stays beside it
        rF = mods_amd.match_pairs(ctxs, imgs1 * stF, imgs2 * stF, pF)
        dtF = time.perf_counter() - ta
        ruF1 = resource.getrusage(resource.RUSAGE_SELF)
        cpuF = (ruF1.ru_utime - ruF0.ru_utime) + (ruF1.ru_stime - ruF0.ru_stime)
        fms, fn, fth = mods_amd.last_batch_verify()
        veF = mods_amd.last_batch_verify_each()      # every pair of that call (stF steps of distinct pairs)
        vst = mods_amd.verify_device_stats()
        import ctypes as _C
        cw, ch = _C.c_double(), _C.c_double()
        mods_amd.lib().modsx_debug_last_batch_cpu(_C.byref(cw), _C.byref(ch))
        tb = time.perf_counter()
        for _ in range(stF):
            mods_amd.match_pairs(ctxs, imgs1, imgs2, pF)
        dtFstep = time.perf_counter() - tb
        wxbs_f = (fms, fn, fth, vst, cw, ch, dtF, dtFstep, cpuF, ruF0, ruF1, rF, stF, veF)
    ladder_parts = {}
    if args.full and ladder and rank == 0 and group is None:
        # the MSER steps alone and the HessianAffine steps alone: the former are short of host CPU, so they too are measured before the
        # contexts have recorded timing events
        for name, det in (("mser_steps_only", 3), ("hessaff_steps_only", 0)):
            st = cviu_ladder_steps(mods_amd, only=det)
            el, nd, _ = timed(lambda st=st: run_batch(steps_l=st), 1, 2)
            ladder_parts[name] = {"pairs_per_s": 2 * nbatch / el, "descriptors_per_pair": nd / (2 * nbatch), "views_per_image": sum(len(v) for v, _, _ in st)}
    elapsed, ndesc_total = reduce_over_ranks(elapsed, ndesc)
    if res is None:   # view-sharded: this rank verified none of the last step's pairs
        res = {"n_regions": (0, 0), "n_tentatives": 0, "n_unique": 0, "n_verified": 0, "H": np.eye(3)}

    # ---- N > 1: the north star's view-parallel mode, measured right after the pair-sharded headline -------------------
    scaling_views = None
    views_hung = False
    guard_flag = None
    if (world > 1 or os.environ.get("MODSX_BENCH_FORCE_VIEWS")) and group is None and not args.no_scaling_views and not single_view and not ladder:
        # The first contact of the RCCL transport with more than one rank must not cost the headline: the measurement runs
        # on a worker thread with a deadline.  Past it (a collective or the communicator bootstrap hangs) every rank reports
        # the pair-sharded line with the error and leaves through os._exit -- no clean-up that could block.
        box = {}
        # ... and a crash must not either: RCCL with more than one rank has only ever run on the driver's node.  Rank 0 leaves
        # the headline with a child process that shares its stdout and prints it if this process dies before its own line.
        if rank == 0 and world > 1:   # never at --gpus 1: the N = 1 line has no leg that could take it away
            pairs0 = args.steps * world * nbatch
            emergency = {
                "metric": "image-pairs/sec (1024x768, HessAff+RootSIFT over the affine view ladder, MFMA FGINN match, LO-RANSAC H)",
                "value": pairs0 / elapsed, "unit": "image-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "f32 (detect/describe) + u8 on the int8 matrix cores (distance matrix)", "data": "synthetic",
                "config": {"workload": "%dx%d synthetic pair, %s = %d views per image, HessAff+RootSIFT, MFMA distance matrix + FGINN, "
                                       "duplicate filter, LO-RANSAC H" % (args.cols, args.rows, cfg_desc, len(views)),
                           "views": len(views), "pairs_per_step": world * nbatch, "workers_per_gpu": len(ctxs),
                           "parallelism": "pairs sharded over ranks, no collective"},
                "descriptors_per_s": ndesc_total / elapsed,
                "scaling_views": {"error": "the process ended during the untimed view-sharded leg; this line was left behind by rank 0 "
                                           "before it started (the legs after it -- roofline, parity, kernel statistics -- did not run)"},
            }
            guard_dir = tempfile.mkdtemp(prefix="modsx_bench_")
            guard_line, guard_flag = os.path.join(guard_dir, "line.json"), os.path.join(guard_dir, "printed")
            with open(guard_line, "w") as f:
                f.write(json.dumps(emergency))
            guard_code = ("import os,sys,time\n"
                          "pid=int(sys.argv[1])\n"
                          "while True:\n"
                          "    try: os.kill(pid,0)\n"
                          "    except OSError: break\n"
                          "    time.sleep(0.2)\n"
                          "if not os.path.exists(sys.argv[3]): sys.stdout.write(open(sys.argv[2]).read()+'\\n'); sys.stdout.flush()\n")
            try:
                subprocess.Popen([sys.executable, "-c", guard_code, str(os.getpid()), guard_line, guard_flag], stdin=subprocess.DEVNULL,
                                 start_new_session=True)
            except OSError:
                guard_flag = None

        def measure_views():
            try:
                if os.environ.get("MODSX_BENCH_CRASH_IN_VIEWS"):   # test hook for the guard above
                    import signal
                    os.kill(os.getpid(), signal.SIGSEGV)
                vhost, vdev = make_images(12345, args.distinct or batch * world, nblobs)       # every rank holds every pair
                nb_v = batch * world
                v1 = [vdev[i % len(vdev)][0] for i in range(nb_v)]
                v2 = [vdev[i % len(vdev)][1] for i in range(nb_v)]
                vg = ShardGroup(mods_amd, local_rank, len(ctxs), dist=dist, ctxs=ctxs, exchange=args.exchange)
                el_v, nd_v, res_v = timed(lambda: vg.step(v1, v2, views, params), max(1, args.warmup), args.steps, vg)
                el_v, nd_v = reduce_over_ranks(el_v, nd_v)
                box["out"] = {"value": args.steps * nb_v / el_v, "unit": "image-pairs/s", "ms_per_step": 1e3 * el_v / args.steps,
                              "pairs_per_step": nb_v, "descriptors_per_s": nd_v / el_v, "scaling": "weak",
                              "parallelism": "views of every pair sharded over %d ranks ((image, view) item f -> rank f mod N), chunks of "
                                             "min(N, 8) pairs per sharded call: ONE RCCL all-gather of header + region rows + u8 descriptors "
                                             "for all image sides of a chunk, ONE all-gather of the result rows of its matching problems "
                                             "(query rows split over the ranks), verification on rank pair mod N" % world,
                              "rccl": vg.describe()}
                vg.close()
                for a_, b_ in vdev:
                    a_.free(); b_.free()
            except Exception as e:       # noqa: BLE001 -- reported in the JSON line, the headline stands
                box["out"] = {"error": "%s: %s" % (type(e).__name__, e)}

        th = threading.Thread(target=measure_views, daemon=True)
        th.start()
        th.join(float(os.environ.get("MODSX_BENCH_VIEWS_DEADLINE_S", "240")))
        if th.is_alive():
            views_hung = True
            scaling_views = {"error": "the view-sharded measurement did not finish within its deadline (hung collective or bootstrap); "
                                      "the process leaves through os._exit after printing this line"}
        else:
            scaling_views = box.get("out")

    # ---- untimed legs (rank 0 reports them) -------------------------------------------------------------------------
    # per-kernel time of the multi-stream regime: an extra step with the event brackets on
    PROF_STEPS = 1
    stats = {}
    pctxs = ctxs
    if views_hung or not args.full:
        pass
    elif (rank == 0 and group is None) or (group is not None and not args.loopback):
        # the event-bracketed legs run on contexts of their own where they can (pair-sharded runs): a context that has recorded timing
        # events costs its host thread more CPU per launch for good (include/modsx.h, modsx_profile), and the legs that follow
        # (`extra`, configs[4]'s and the ladder's parts) are measured on the timed region's contexts
        if group is None:
            pctxs = [mods_amd.Context(local_rank) for _ in ctxs]
        for c in pctxs:
            c.profile(True)
        for _ in range(PROF_STEPS):
            run_batch(cx=pctxs)
        barrier(group) if group is not None else [c.synchronize() for c in pctxs]
        for c in pctxs:
            for k, v in c.kernel_stats().items():
                d = stats.setdefault(k, dict(ms=0.0, work=0.0, launches=0))
                d["ms"] += v["ms"]; d["work"] += v["work"]; d["launches"] += v["launches"]
            c.profile(False)
    # Roofline leg: in the timed region the kernels of --workers streams time-slice the CUs, so an event pair there
    # brackets queueing as well.  The same pairs are repeated on ONE stream and the launch durations come from that pass.
    iso, niso, mroof = {}, 0, None
    if args.full and rank == 0 and not views_hung and (group is None or views_world == 1 or args.loopback):
        # really one stream: a lone multi-view pair would otherwise run image 2 on a peer context and every image in three parts on
        # helper contexts (engine_views.hip), and the event brackets of this leg would include their queueing
        os.environ["MODSX_PAIR_SERIAL"] = "1"; os.environ["MODSX_PAIR_NOSPLIT"] = "1"
        pctx = pctxs[0]
        pctx.profile(True)
        niso = min(nbatch, 8 if single_view else 4)
        if single_view:
            for i0 in range(0, niso, 4):
                mods_amd.match_pairs([pctx], imgs1[i0:min(i0 + 4, niso)], imgs2[i0:min(i0 + 4, niso)], params)
        else:
            for i in range(niso):
                pctx.match_pair_views(imgs1[i], imgs2[i], views, params)
        pctx.synchronize()
        iso = {k: v for k, v in pctx.kernel_stats().items() if v["launches"]}
        pctx.profile(False)
        if not single_view:
            # the matcher's roofline: ONE pair (pair 0), repeated; N, M and the work all come from that pair
            pctx.profile(True)
            REP = 5
            for _ in range(REP):
                r0 = pctx.match_pair_views(imgs1[0], imgs2[0], views, params)
            pctx.synchronize()
            ks = pctx.kernel_stats()
            m, m1 = ks.get("match_fginn"), ks.get("match_sweep1")
            pctx.profile(False)
            if m and m["launches"]:
                mroof = (m["ms"] / m["launches"], r0["n_regions"][0], r0["n_regions"][1], m["launches"],
                         m1["ms"] / m1["launches"] if m1 and m1["launches"] else None)
        os.environ.pop("MODSX_PAIR_SERIAL", None); os.environ.pop("MODSX_PAIR_NOSPLIT", None)
    if pctxs is not ctxs:
        for c in pctxs:
            c.close()

    if rank == 0:
        pairs = args.steps * (nbatch if group is not None else world * nbatch)
        value = pairs / elapsed
        out = {
            "metric": "image-pairs/sec (1024x768, HessAff+RootSIFT over the affine view ladder, MFMA FGINN match, LO-RANSAC H)",
            "value": value, "unit": "image-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32 (detect/describe) + u8 on the int8 matrix cores (distance matrix)", "data": "synthetic",
            "config": {"workload": ("%dx%d synthetic pair, %s, MSER + HessAff, RootSIFT, MFMA distance matrix + FGINN per class, duplicate "
                                    "filter, LO-RANSAC H after every step" % (args.cols, args.rows, cfg_desc)) if ladder else
                                   ("%dx%d synthetic pair, %s = %d views per image, HessAff+RootSIFT, MFMA distance matrix + "
                                    "FGINN, duplicate filter, LO-RANSAC H" % (args.cols, args.rows, cfg_desc, len(views))),
                       "views": len(views), "pairs_per_step": nbatch if group is not None else world * nbatch,
                       "workers_per_gpu": len(ctxs), "distinct_pairs": len(dev), "blobs_per_1024x768": blobs,
                       "parallelism": ("views of every pair sharded over %d ranks (v mod N), one all-gather of header + region rows + u8 "
                                       "descriptors per image side (%s), query rows of the match split over ranks"
                                       % (views_world, "loopback transport, all ranks on this GPU" if args.loopback else "RCCL"))
                                      if group is not None else "pairs sharded over ranks, no collective"},
            "descriptors_per_s": ndesc_total / elapsed,
            "descriptors_per_pair": ndesc_total / pairs,
            "result": {"regions": list(res["n_regions"]), "tentatives": res["n_tentatives"], "unique": res["n_unique"],
                       "verified": res["n_verified"],
                       "H_vs_generator_max_abs": float(np.abs(res["H"] / res["H"][2, 2] - Hgt).max())},
        }
        if stats:
            out["kernel_ms_per_pair_multi_stream"] = {k: v["ms"] / (PROF_STEPS * nbatch) for k, v in stats.items() if v["launches"]}
        # the same figure under a key that never changes meaning: with N > 1 `value` becomes the view-sharded one (below)
        out["value_pair_sharded"] = value
        out["steps_issue"] = ("back to back: a context goes from the last pair of step k to the first of step k + 1, no host-side barrier "
                              "between the K timed steps (barrier + synchronize before the first and after the last)") if b2b else \
                             "a host-side barrier after every step"
        if barrier_form is not None:
            out["value_with_step_barrier"] = barrier_form
        out["upload_in_timed_region"] = False      # inputs are resident in HBM when the timed region starts (the bench contract)
        if upload_form is not None:
            out["value_with_upload"] = upload_form
        out["config"]["image_generation_s"] = round(t_gen, 2)
        if host_cpu.get("s") is not None:
            # rank 0's own threads (workers, verification helpers, host pool) over its share of the timed pairs: on a node where N ranks
            # share one host, N times this figure per second of throughput is what the host has to supply
            out["host_cpu_s_per_pair_rank0"] = host_cpu_headline / max(1, args.steps * nbatch)
            try:
                out["host_wait"] = (os.environ.get("MODSX_HOST_WAIT") or "auto (by CPU load: flag word + naps when the process uses > 80 % of its CPU allowance, the runtime's wait below 60 %)") + "; at the end of the run: " + ("runtime" if mods_amd.lib().modsx_debug_host_wait_runtime() else "flag")
            except Exception:
                pass
            if b2b and host_cpu_split[0] > 0:
                npz = max(1, args.steps * nbatch)
                out["host_cpu_split_s_per_pair"] = {"context_threads": host_cpu_split[0] / npz, "other_threads": (host_cpu_headline - host_cpu_split[0]) / npz,
                                                    "of_which_system_time": host_cpu_split[1] / npz,
                                                    "note": "context_threads = the threads that drive the contexts (thread CPU clocks); other_threads = verification helpers, "
                                                            "host pool and the HIP / HSA runtime's own threads; system time = all threads"}
            allowance, lranks = cpu_info()[2], int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
            out["host_threads"] = {"cpu_allowance": allowance, "local_ranks": lranks}
            # what the host can feed: the node's CPU allowance over the CPU-seconds a pair costs a rank's threads.  With N ranks on one
            # host the allowance is shared: host_limited says that the measured (or, at N = 1, the N-fold) throughput is at that bound
            hb = allowance / max(out["host_cpu_s_per_pair_rank0"], 1e-9)
            out["host_bound_pairs_per_s"] = hb
            out["host_limited"] = bool(value >= 0.9 * hb)
            out["host_bound_note"] = ("cpu_allowance / host_cpu_s_per_pair_rank0 for the whole node: %d CPUs feed at most %.0f pairs/s of this workload, "
                                      "i.e. %.1f GPUs at this run's per-GPU rate; host_limited = the job's value is within 10 %% of that bound"
                                      % (allowance, hb, hb / max(value / max(1, world), 1e-9)))
        if group is not None:
            out["rccl"] = group.describe()
        if scaling_views is not None:
            out["scaling_views"] = scaling_views
            if world > 1 and "value" in scaling_views:
                # N > 1: the headline is the north star's mode -- views of every pair sharded over the ranks, RCCL all-gathers of
                # region rows + descriptors and of the result rows -- so that a scaling run exercises the collectives; the
                # pair-sharded figure (independent pairs per rank, no collective) measured just before it stays beside it.  (Had
                # the view-sharded leg failed, hung or crashed, the line would carry the pair-sharded value and the error.)
                out["pair_sharded"] = {"value": out["value"], "unit": "image-pairs/s", "ms_per_step": out["ms_per_step"],
                                       "pairs_per_step": out["config"]["pairs_per_step"], "descriptors_per_s": out["descriptors_per_s"],
                                       "parallelism": out["config"]["parallelism"]}
                out["value"] = scaling_views["value"]
                out["ms_per_step"] = scaling_views["ms_per_step"]
                out["descriptors_per_s"] = scaling_views["descriptors_per_s"]
                out["config"]["pairs_per_step"] = scaling_views["pairs_per_step"]
                out["config"]["parallelism"] = scaling_views["parallelism"]
                out["rccl"] = scaling_views.get("rccl")
                out["headline_mode"] = "views sharded over ranks (RCCL); pair_sharded = the no-collective figure of the same run"
        if iso:
            per = {k: v["ms"] / niso for k, v in iso.items()}
            out["kernels_single_stream_ms_per_pair"] = per
            if mroof is None and iso.get("match_fginn", {}).get("launches"):
                m = iso["match_fginn"]      # configs[1] / [4]: launch sets of 4 small problems; per launch set
                mroof = (m["ms"] / m["launches"], None, None, m["launches"], None)
                flops = m["work"] / m["launches"]
            if mroof is not None:
                ms, n1, n2, nl, ms1 = mroof
                if n1 is not None:
                    flops = 2.0 * n1 * n2 * 128
                tf = flops / (ms * 1e-3) / 1e12
                out["roofline"] = {
                    "kernel": "k_match_* (every launch of one matching problem: pack, sweep 1, decide, resolve)",
                    "bound": "mfma", "achieved": tf, "peak": INT8_PEAK_TOPS, "unit": "TFLOP/s", "frac": tf / INT8_PEAK_TOPS,
                    "traffic": None, "avg_launch_ms": ms, "algorithmic_work_per_launch": flops, "N": n1, "M": n2,
                    "binds": "mfma: 2*N*M*128 int8 ops against (N+M)*128 B is ~1e4 op/B, the kernel is compute-shaped; "
                             "sweep 1 carries the contraction; pack / decide / resolve are latency chains (DESIGN.md section 5.6)",
                    "note": ("HIP events on the launch stream around the launches of ONE matching problem -- pair 0 of this run, "
                             "%d repetitions on one stream right after the timed region; N, M, the work and the time all belong "
                             "to that pair" % nl) if n1 is not None else
                            "HIP events on the launch stream; one launch set = up to 4 small problems, work = their sum"}
                if n1 is not None:
                    byts = (n1 + n2) * 128.0 + n1 * 32.0
                    out["roofline"]["hbm_view"] = {"compulsory_bytes": byts, "achieved_GBs": byts / (ms * 1e-3) / 1e9,
                                                   "frac_of_8TBs": byts / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
                if ms1:
                    tf1 = flops / (ms1 * 1e-3) / 1e12
                    out["roofline_sweep1"] = {
                        "kernel": "k_match_sweep1 alone: the one launch that carries the 2*N*M*128 contraction of the problem above "
                                  "(k_match_resolve repeats about 1 % of it for the undecided queries; pack / decide issue no MFMA)",
                        "bound": "mfma", "achieved": tf1, "peak": INT8_PEAK_TOPS, "unit": "TFLOP/s", "frac": tf1 / INT8_PEAK_TOPS,
                        "avg_launch_ms": ms1, "algorithmic_work_per_launch": flops, "traffic": None,
                        "measured_ceilings_TOPs": {"mfma_only_descriptor_like_operands": 3800.0, "with_the_top2_reduction_VALU": 3000.0,
                                                   "source": "profiles/r03_ubench_mfma.txt (tools/ubench/mfma_chain_sift, mfma_lds)"},
                        "note": "HIP events on the launch stream around k_match_sweep1 of the same %d repetitions" % nl}
            tfile, tsrc = None, None
            for tag in ("r06", "r05", "r04", "r03", "r02"):
                cand = os.path.join(ROOT, "profiles", "pmc_traffic_%s.json" % tag)
                if os.path.exists(cand):
                    tfile, tsrc = cand, "profiles/pmc_traffic_%s.json" % tag
                    break
            tj = json.load(open(tfile)) if tfile else {}
            if "roofline" in out and tj:
                out["roofline"]["traffic"] = tj.get("k_match_total_views31")
                if tj.get("k_match_total_views31") and tj.get("k_match_compulsory_bytes"):
                    out["roofline"]["traffic_over_compulsory"] = tj["k_match_total_views31"] / tj["k_match_compulsory_bytes"]
                if tj.get("hbm_counter_GB_per_pair"):
                    out["hbm_counter_GB_per_pair"] = tj["hbm_counter_GB_per_pair"]      # whole pipeline, one stream, same profile
                out["roofline"]["traffic_source"] = ("%s: FETCH_SIZE x2 + WRITE_SIZE of the k_match_* kernels from separate rocprofv3 --pmc "
                                                     "passes over tools/bench_match.py at %s (a committed profile, not measured in this run)"
                                                     % (tsrc, tj.get("k_match_problem", "24.1 k x 23.6 k real 31-view descriptors")))
            dk = [iso.get(k) for k in ("patch_sample", "blur_rows", "blur_cols", "describe")]
            if all(d and d["launches"] for d in dk):
                ms = sum(d["ms"] for d in dk) / dk[0]["launches"]
                byts = (dk[0]["work"] + dk[3]["work"]) / dk[0]["launches"]
                out["roofline_describe"] = {
                    "kernel": "describe stage: k_sample_rows_lds (sampling fused with the row filter; k_patch_sample + k_patch_blur for the few windows beyond LDS) + k_blur_cols_lds + k_describe (one chunk = one launch of each)",
                    "bound": "hbm", "achieved": byts / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": byts / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "avg_launch_ms": ms,
                    "algorithmic_work_per_launch": byts, "traffic": None,
                    "note": "bytes per SURVEY section 8(d): (P+2)^2 x 4 B read + 128 B written per region; the limiter of these "
                            "kernels is VALU issue / the texture addresser, not HBM (DESIGN.md section 5)"}
                if tj:
                    # HBM bytes (FETCH_SIZE x 2 + WRITE_SIZE, rocprofv3 --pmc, separate passes) of one launch of each kernel of the stage
                    # in the PROFILED run, whose chunks differ in size from this run's: scaled by the ratio of the two chunks'
                    # algorithmic bytes so that traffic and algorithmic_work_per_launch describe the same launch
                    tprof = sum(tj.get(k, 0) for k in ("k_sample_rows_lds", "k_patch_sample", "k_blur_rows_lds",
                                                       "k_patch_blur", "k_blur_cols_lds", "k_describe")) or None
                    aprof = tj.get("describe_chunk_algorithmic_bytes", 163.0e6)
                    out["roofline_describe"]["traffic"] = tprof * byts / aprof if tprof else None
                    out["roofline_describe"]["traffic_over_algorithmic"] = tprof / aprof if tprof else None
                    out["roofline_describe"]["traffic_source"] = ("%s: %.0f MB per chunk of %.0f MB algorithmic bytes in the committed one-stream "
                                                                  "31-view profile, scaled to this run's chunk (x %.3f)"
                                                                  % (tsrc, (tprof or 0) / 1e6, aprof / 1e6, byts / aprof))
        if wxbs and wxbs_f:
            # H verification was the timed region; the same batch with epipolar verification, and the host share of both
            vms, vn, vth = verify_timed
            hshare = {"verify_ms_per_pair": vms / max(1, vn), "helper_threads": vth}
            (fms, fn, fth, vst, cw, ch, dtF, dtFstep, cpuF, ruF0, ruF1, rF, stF, veF) = wxbs_f
            def _mmm(x):
                x = np.sort(np.asarray(x, float))
                return {"min": float(x[0]), "median": float(x[len(x) // 2]), "max": float(x[-1]), "pairs": int(len(x))} if len(x) else None
            hshare["verify_ms_per_pair_min_median_max"] = _mmm(verify_each_h)
            out["wxbs"] = {
                "H": {"pairs_per_s": value, **hshare,
                      "host_ransac_share_of_wall": (vms / max(1, vn)) / max(1, vth) / (1e3 / value) * 1.0},
                "F": {"pairs_per_s": stF * nbatch / dtF, "pairs_per_s_one_call_per_step": stF * nbatch / dtFstep, "verify_ms_per_pair": fms / max(1, fn), "helper_threads": fth,
                      "verify_ms_per_pair_min_median_max": _mmm(veF),
                      "verified_last_pair": rF[0]["n_verified"], "host_cpu_s_per_pair": cpuF / (stF * nbatch),
                      "host_cores_busy": cpuF / dtF, "cpu_s_per_pair_context_threads": cw.value / (stF * nbatch),
                      "cpu_s_per_pair_verification_helpers": ch.value / (stF * nbatch), "host_cpu_system_share": (ruF1.ru_stime - ruF0.ru_stime) / max(cpuF, 1e-9),
                      "rfth_loops_per_pair": vst["loops"] / float(stF * nbatch), "rfth_ms_per_loop": 1e-3 * vst["loop_us"] / max(1, vst["loops"]),
                      "rfth_ms_per_loop_parts": {k: 1e-3 * vst[k + "_us"] / max(1, vst["loops"]) for k in ("draw", "device_wait", "host_phase", "event_body")},
                      "rfth_hypotheses_on_device": vst["hypotheses"], "rfth_device_batches": vst["batches"],
                      "host_ransac_share_of_wall": (fms / max(1, fn)) / max(1, fth) / (dtF / (stF * nbatch) * 1e3)},
                "note": "DuplicateFiltering + LO-RANSAC run on helper threads beside the device pipeline; share = per-pair verify "
                        "time / helper threads / per-pair wall time (the fraction of the wall the helpers are busy)"}
        if ladder and args.full:
            # where a ladder's time goes: the MSER steps alone and the HessianAffine steps alone (throughput, same contexts), and
            # one pair on an otherwise idle GPU step by step (latency)
            lad = {"steps": [{"detector": "MSER" if d == 3 else "HessianAffine", "views": len(v), "match_ratio": r} for v, r, d in lsteps]}
            lad.update(ladder_parts)        # measured right after the timed region (see wxbs_f above: before any event-bracketed leg)
            lat = []
            ctx.match_ladder(imgs1[0], imgs2[0], lsteps, params, min_matches=10 ** 6)
            for k in range(1, len(lsteps) + 1):
                ta = time.perf_counter()
                for _ in range(3):
                    ctx.match_ladder(imgs1[0], imgs2[0], lsteps[:k], params, min_matches=10 ** 6)
                lat.append((time.perf_counter() - ta) / 3 * 1e3)
            lad["one_pair_idle_gpu_ms_cumulative_by_step"] = lat
            lad["one_pair_idle_gpu_ms_by_step"] = [lat[0]] + [lat[k] - lat[k - 1] for k in range(1, len(lat))]
            lad["host_threads"] = os.environ.get("MODSX_HOST_THREADS", "min(hardware threads, cgroup CPU allowance, 64) / local ranks")
            lad["note"] = ("the component trees of the MSER steps run on the host worker pool ((view, polarity) tasks) while other "
                           "contexts keep the device busy; mser_steps_only / hessaff_steps_only are the same contexts on a ladder cut to "
                           "that detector's steps")
            out["ladder"] = lad
        # ---- short runs of the other view counts (same timed-region rules, fewer steps) ---------------------------------
        if args.full and not args.no_extra and group is None and world == 1 and not args.tilts and not wxbs and not ladder:
            extra = {}
            for name in ("views1", "views8", "views11"):
                if name == args.config:
                    continue
                tl, ph, _ = CONFIGS[name]
                vw = mods_amd.set_vs_pars([1.0], [float(t) for t in tl.split(",")], ph, args.init_sigma, 1, [])
                nb = 256 if tl == "1" else 64
                i1 = [dev[i % len(dev)][0] for i in range(nb)]
                i2 = [dev[i % len(dev)][1] for i in range(nb)]
                el, nd, _ = timed(lambda: run_batch(vw, tl == "1", i1, i2), 1, 3)
                extra[name] = {"views": len(vw), "pairs_per_s": 3 * nb / el, "descriptors_per_pair": nd / (3 * nb),
                               "descriptors_per_s": nd / el, "blobs_per_1024x768": blobs}
            if not args.blobs and not single_view:
                # the scene of SURVEY section 8(d) item 2 (4000 blobs per 1024x768) under the headline's view ladder
                h4, d4 = make_images(12345, distinct, int(4000 * args.rows * args.cols / (768.0 * 1024)))
                i1 = [d4[i % len(d4)][0] for i in range(nbatch)]
                i2 = [d4[i % len(d4)][1] for i in range(nbatch)]
                el, nd, _ = timed(lambda: run_batch(views, False, i1, i2), 1, 3)
                extra["%s_4000_blobs" % args.config] = {"views": len(views), "pairs_per_s": 3 * nbatch / el, "descriptors_per_pair": nd / (3 * nbatch),
                                                        "descriptors_per_s": nd / el, "blobs_per_1024x768": 4000}
                for a_, b_ in d4:
                    a_.free(); b_.free()
                # configs[2] with a scene dense enough that the per-view costs (synthesis, pyramid) are amortised over more regions:
                # 8 views, 16000 blobs per 1024x768 -- the configuration in which the path delivers its most descriptors per second
                h8, d8 = make_images(12345, min(distinct, 64), int(16000 * args.rows * args.cols / (768.0 * 1024)))
                tl, ph, _ = CONFIGS["views8"]
                vw = mods_amd.set_vs_pars([1.0], [float(t) for t in tl.split(",")], ph, args.init_sigma, 1, [])
                i1 = [d8[i % len(d8)][0] for i in range(64)]
                i2 = [d8[i % len(d8)][1] for i in range(64)]
                el, nd, _ = timed(lambda: run_batch(vw, False, i1, i2), 1, 3)
                extra["views8_16000_blobs"] = {"views": len(vw), "pairs_per_s": 3 * 64 / el, "descriptors_per_pair": nd / (3 * 64),
                                               "descriptors_per_s": nd / el, "blobs_per_1024x768": 16000}
                # 16 views (TiltSet 1,2,3,4,6, Phi 180) of a dense scene (20000 blobs): >= 50 k descriptors per pair again, from half the
                # views of the headline -- what the per-view costs (view synthesis, pyramid: ~22 % of the headline's kernel time) weigh
                for a_, b_ in d8:
                    a_.free(); b_.free()
                h16, d16 = make_images(12345, min(distinct, 64), int(20000 * args.rows * args.cols / (768.0 * 1024)))
                vw16 = mods_amd.set_vs_pars([1.0], [1.0, 2.0, 3.0, 4.0, 6.0], 180.0, args.init_sigma, 1, [])
                i1 = [d16[i % len(d16)][0] for i in range(64)]
                i2 = [d16[i % len(d16)][1] for i in range(64)]
                el, nd, _ = timed(lambda: run_batch(vw16, False, i1, i2), 1, 3)
                extra["views16_20000_blobs"] = {"views": len(vw16), "pairs_per_s": 3 * 64 / el, "descriptors_per_pair": nd / (3 * 64),
                                                "descriptors_per_s": nd / el, "blobs_per_1024x768": 20000}
                for a_, b_ in d16:
                    a_.free(); b_.free()
            out["extra"] = extra
        # ---- the CPU path on the same workload: parity of one pair of the run + the baseline timing ---------------------
        if args.full and world == 1 and not args.no_cpu_baseline and not wxbs and not ladder and group is None:
            from oracle import pyoracle as O
            model, ncpu, usable = cpu_info()
            a, b = pairs_host[0][0].astype(np.float32), pairs_host[0][1].astype(np.float32)
            vo = O.set_vs_pars([1.0], [float(t) for t in tilts.split(",")], phi, args.init_sigma, 1, [])
            O.detect_describe_views(a[:64, :64].copy(), vo[:1])     # lazy tables (single-threaded once)
            full = oracle_pair_views(O, a, b, vo, params, threads=usable, seed=1)
            got = ctx.match_pair_views(imgs1[0], imgs2[0], views, params)
            par = {"pair": "pair 0 of the run, GPU path vs CPU oracle",
                   "regions_identical": bool(got["n_regions"] == (len(full["regs"][0]), len(full["regs"][1]))),
                   "tentatives_identical": bool(got["n_unique"] == len(full["uniq"]) and all(
                       np.array_equal(got["tentatives"][f], full["uniq"][f]) for f in ("q", "t0", "tj", "t1", "d1", "d2", "ratio")))}
            if full["ransac"] is not None:
                par["inliers_identical"] = bool(np.array_equal(got["ransac_inlier"], full["ransac"]["inl"]))
                Hc = np.asarray(full["ransac"]["H"], float).reshape(3, 3)
                par["H_vs_cpu_max_abs"] = float(np.abs(got["H"] / got["H"][2, 2] - Hc / Hc[2, 2]).max())
            out["parity"] = par
            # one thread: a bounded sample (image A's views + 2048 query rows of the match), scaled to a full pair
            s1 = oracle_pair_views(O, a, b, vo, params, threads=1, one_image=True)
            try:
                import ctypes
                ctypes.CDLL("libgomp.so.1").omp_set_num_threads(1)
            except OSError:
                pass
            nq = min(2048, len(full["desc"][0]))
            pos2 = np.stack([full["regs"][1]["reproj_kp"]["x"], full["regs"][1]["reproj_kp"]["y"]], 1)
            tm = time.time()
            O.match_fginn(full["desc"][0][:nq], full["desc"][1], pos2, params.match_ratio, params.contradDist)
            tm = time.time() - tm
            n1 = len(full["desc"][0])
            est = 2 * s1["t_extract"] + tm * n1 / nq + full["t_verify"]
            base = {"value": 1.0 / full["total"], "unit": "image-pairs/s", "cores": usable, "kind": "port",
                    "cpu_model": model, "host_logical_cpus": ncpu,
                    "cores_note": "threads = the container's CPU allowance (cgroup cpu.max) when it is below the visible CPUs",
                    "matcher_note": "the restatement matches with the exact linear kNN (the parity target); the reference's shipped "
                                    "configs use a randomised kd-tree (config_iter_mods_cviu.ini:132), which is cheaper -- the match share "
                                    "of this baseline overstates the reference's cost",
                    "sample": "1 full pair of this workload (%d views per image, %d + %d regions) on %d threads in %.2f s: "
                              "(image, view) tasks on a thread pool as the reference's OpenMP loops (mods.cpp:255-271, "
                              "imagerepresentation.cpp:612-622), OpenMP over the query rows of the linear kNN; extract %.2f s, "
                              "match %.2f s, duplicate filter + reference degensac %.2f s"
                              % (len(views), len(full["regs"][0]), len(full["regs"][1]), usable, full["total"],
                                 full["t_extract"], full["t_match"], full["t_verify"]),
                    "descriptors_per_s": (len(full["regs"][0]) + len(full["regs"][1])) / full["total"],
                    "single_thread": {"value": 1.0 / est, "unit": "image-pairs/s", "cores": 1,
                                      "sample": "image A's %d views (%.1f s, doubled) + %d of %d query rows of the match (%.1f s, "
                                                "scaled) + verification of the full pair (%.2f s) -> %.1f s per pair"
                                                % (len(views), s1["t_extract"], nq, n1, tm, full["t_verify"], est)}}
            # the one stage where the real reference runs here: degensac from oracle/_ref vs the product's host C++
            if full["ransac"] is not None and len(full["pts"]) >= 8:
                tr = time.time()
                for _ in range(3):
                    O.loransac_h(full["pts"], full["laf1"], full["laf2"], err_threshold=params.err_threshold,
                                 confidence=params.confidence, max_samples=params.max_samples, seed=1)
                tr = (time.time() - tr) / 3
                tp = time.time()
                for _ in range(3):
                    mods_amd.loransac_h(full["pts"], full["laf1"], full["laf2"], err_threshold=params.err_threshold,
                                        confidence=params.confidence, max_samples=params.max_samples, seed=1)
                tp = (time.time() - tp) / 3
                base["ransac_reference_vs_restatement"] = {
                    "reference_degensac_ms": 1e3 * tr, "libmodsx_host_ms": 1e3 * tp, "ratio": tr / tp if tp > 0 else None,
                    "tentatives": int(len(full["pts"])),
                    "note": "LORANSACFiltering (H) on the tentatives of this pair: the reference's own degensac C sources "
                            "(oracle/_ref, built in the build container) vs the restatement shipped in libmodsx"}
            out["cpu_baseline"] = base
        else:
            out["cpu_baseline"] = None
        # RCCL writes a version banner through C stdio, which would otherwise be flushed at exit, after this line
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stdout.flush()
        # --gpus N must mean N ranks in ONE RCCL communicator: anything else (a bootstrap that fell back to per-rank worlds, a launcher
        # that started fewer ranks) is an error in the line and in the exit code, not a smaller number that looks like a result
        rc_info = out.get("rccl") or {}
        if args.gpus and args.gpus != world and not args.loopback:
            out["error"] = "--gpus %d, but the launcher started %d rank(s) (WORLD_SIZE)" % (args.gpus, world)
            exit_code = 3
        elif world > 1 and not args.loopback and rc_info.get("ranks_seen_by_rccl") != world:
            out["error"] = ("--gpus %d, but the RCCL communicator holds %s ranks (transport %s): the view-sharded figure is not a %d-GPU "
                            "measurement" % (world, rc_info.get("ranks_seen_by_rccl"), rc_info.get("transport"), world))
            exit_code = 3
        if guard_flag:
            open(guard_flag, "w").close()     # from here on the line is this process's to print
        print(json.dumps(out), flush=True)
    if views_hung:
        sys.stdout.flush()
        os._exit(exit_code or 0)
    for a_, b_ in dev:
        a_.free(); b_.free()
    if group is not None:
        group.close()
    for c in ctxs:
        c.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if exit_code:
        sys.exit(exit_code)


if __name__ == "__main__":
    main()
