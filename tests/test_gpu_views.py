"""GPU: view synthesis and the multi-view loop against the oracle (bit-exact)."""
import os

import numpy as np
import pytest

from common import laf_of, normH, oracle_ladder, same_records, need_ref, check_batch_statistics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _views(oracle, modsx, tilts, phi, sigma=0.2):
    vo = oracle.set_vs_pars([1.0], tilts, phi, sigma, 1, [])
    vm = modsx.set_vs_pars([1.0], tilts, phi, sigma, 1, [])
    return vo, vm


@pytest.mark.parametrize("tilt,phi,zoom,sigma,blur", [
    (2.0, 0.0, 1.0, 0.2, 1), (4.0, np.pi / 2, 1.0, 0.2, 1), (6.0, 2 * np.pi / 3, 1.0, 0.5, 1), (3.0, 0.0, 0.5, 0.5, 1),
    (-2.0, 0.0, 1.0, 0.5, 1), (8.0, 1.0, 1.0, 0.5, 1), (1.0, 0.0, 0.7, 0.5, 1), (1.0, 0.0, 1.0, 0.5, 1),
    # beyond the fused rotate + blur kernel's halo (the separate launches): a tall column filter (vertical tilt), a row
    # filter of 73 taps; the widest halo the fused kernel takes (49 taps); no blur at all
    (-6.0, 0.3, 1.0, 0.8, 1), (8.0, 0.7, 1.0, 3.0, 1), (8.0, 2.0, 1.0, 2.0, 1), (4.0, 1.2, 1.0, 0.5, 0)])
def test_synth_view_bit_exact(ctx, modsx, oracle, small_pair, tilt, phi, zoom, sigma, blur):
    a = small_pair[0]
    im = ctx.upload(a)
    vo = oracle.make_view(tilt, phi, zoom, sigma, blur)
    vm = modsx.make_view(tilt, phi, zoom, sigma, blur)
    ref, Href, ident_ref = oracle.synth_view(a, vo)
    got, H, ident = ctx.synth_view(im, vm)
    assert ident == ident_ref and np.array_equal(H, Href)
    assert (got.rows, got.cols) == ref.shape
    assert np.array_equal(got.download(), ref)
    got.free(); im.free()


def test_detect_describe_views_bit_exact(ctx, modsx, oracle, small_pair):
    a = small_pair[0]
    im = ctx.upload(a)
    vo, vm = _views(oracle, modsx, [1, 2, 3, 4, 6], 360.0)
    assert len(vm) == 8
    regs_ref, desc_ref = oracle.detect_describe_views(a, vo)
    regs, desc = ctx.detect_describe_views(im, vm, modsx.default_pair_params())
    assert len(regs_ref) > 300
    assert same_records(regs, regs_ref.view(modsx.REGION))
    assert np.array_equal(desc, desc_ref)
    # a shard (every 2nd view starting at 1) equals the corresponding view blocks, ids local to the block
    r2, d2 = ctx.detect_describe_views(im, vm, modsx.default_pair_params(), view_begin=1, view_step=2)
    sel = np.isin(regs_ref["img_id"], [1, 3, 5, 7])
    assert len(r2) == sel.sum() and np.array_equal(d2, desc_ref[sel])
    assert np.array_equal(r2["reproj_kp"]["x"], regs_ref["reproj_kp"]["x"][sel])
    im.free()


def test_pair_views_end_to_end(ctx, modsx, oracle, small_pair):
    a, b, H = small_pair
    need_ref(oracle)
    vo, vm = _views(oracle, modsx, [1, 2, 3], 360.0)
    ia, ib = ctx.upload(a), ctx.upload(b)
    got = ctx.match_pair_views(ia, ib, vm, modsx.default_pair_params(ransac_seed=4))
    r1, d1 = oracle.detect_describe_views(a, vo)
    r2, d2 = oracle.detect_describe_views(b, vo)
    assert got["n_regions"] == (len(r1), len(r2))
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    tent = oracle.match_fginn(d1, d2, pos2, 0.8, 30.0)
    assert got["n_tentatives"] == len(tent)
    pts = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                    r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = oracle.duplicate_filtering(pts, tent["ratio"], 2.0, True)
    sel = order[keep]
    tu, pu = tent[sel], pts[sel]
    for f in tu.dtype.names:
        assert np.array_equal(got["tentatives"][f], tu[f]), f
    rr = oracle.loransac_h(pu, laf_of(r1, tu["q"]), laf_of(r2, tu["t0"]), seed=4)
    assert np.array_equal(got["ransac_inlier"], rr["inl"]) and np.array_equal(got["verified"], rr["keep"])
    assert np.abs(normH(got["H"]) - normH(rr["H"])).max() < 1e-4
    assert np.abs(normH(got["H"]) - H).max() < 1.5
    ia.free(); ib.free()


def test_configs2_eight_views_full_size_end_to_end(ctx, modsx, oracle):
    """configs[2] as BASELINE.json states it: the 1024x768 synthetic pair under TiltSet 1,2,3,4,6 / Phi 360 (8 views,
    SURVEY.md section 8(d) item 3) through ONE match_pair_views call -- region counts, every unique tentative, the inlier set,
    the verified set and H against the oracle's loop over the same views."""
    import os
    from mods_amd import synthetic
    need_ref(oracle)
    a, b, H = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
    vo, vm = _views(oracle, modsx, [1, 2, 3, 4, 6], 360.0)
    assert len(vm) == 8
    ia, ib = ctx.upload(a), ctx.upload(b)
    got = ctx.match_pair_views(ia, ib, vm, modsx.default_pair_params(ransac_seed=4))
    ia.free(); ib.free()
    th = min(64, os.cpu_count() or 1)
    r1, d1 = oracle.detect_describe_views(a, vo, threads=th)
    r2, d2 = oracle.detect_describe_views(b, vo, threads=th)
    assert got["n_regions"] == (len(r1), len(r2)) and len(r1) > 8000
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    tent = oracle.match_fginn(d1, d2, pos2, 0.8, 30.0)
    assert got["n_tentatives"] == len(tent) and len(tent) > 1000
    pts = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                    r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = oracle.duplicate_filtering(pts, tent["ratio"], 2.0, True)
    sel = order[keep]
    tu, pu = tent[sel], pts[sel]
    for f in tu.dtype.names:
        assert np.array_equal(got["tentatives"][f], tu[f]), f
    rr = oracle.loransac_h(pu, laf_of(r1, tu["q"]), laf_of(r2, tu["t0"]), seed=4)
    assert np.array_equal(got["ransac_inlier"], rr["inl"]) and np.array_equal(got["verified"], rr["keep"])
    assert np.abs(normH(got["H"]) - normH(rr["H"])).max() < 1e-4
    assert np.abs(normH(got["H"]) - H).max() < 1.5


CAT_CENTRE_TOL_PX, CAT_CORNER_TOL_PX = 15.0, 75.0   # transfer error of the recovered H against build/examples/cat.txt over the support of the matches


def test_cat_pair_with_views_recovers_ground_truth(ctx, modsx, cat_pair):
    """The example pair of the reference (build/examples/cat.png, cat2.png) needs synthesised views; with the
    HessianAffine ladder of iters_mods_cviu.ini step 4 (TiltSet 1,2,4,6,8, Phi 360, initSigma 0.2) the verified
    homography must agree with the shipped ground truth build/examples/cat.txt."""
    cat, cat2, Hgt = cat_pair
    i1, i2 = ctx.upload(cat), ctx.upload(cat2)
    views = modsx.set_vs_pars([1.0], [1, 2, 4, 6, 8], 360.0, 0.2, 1, [])
    par = modsx.default_pair_params(ransac_seed=3)
    got = ctx.match_pair_views(i1, i2, views, par)
    r1, _ = ctx.detect_describe_views(i1, views, par, want_desc=False)
    r2, _ = ctx.detect_describe_views(i2, views, par, want_desc=False)
    i1.free(); i2.free()
    assert got["n_regions"] == (len(r1), len(r2))
    assert got["n_verified"] >= 15                                   # minMatches of the reference configs
    t = got["tentatives"][got["verified"]]
    p1 = np.stack([r1["reproj_kp"]["x"][t["q"]], r1["reproj_kp"]["y"][t["q"]], np.ones(len(t))], 1)
    p2 = np.stack([r2["reproj_kp"]["x"][t["t0"]], r2["reproj_kp"]["y"][t["t0"]]], 1)
    proj = p1 @ normH(Hgt).T
    proj = proj[:, :2] / proj[:, 2:]
    err = np.linalg.norm(proj - p2, axis=1)
    # the verified correspondences obey the shipped ground-truth homography (cat.txt)
    assert np.mean(err < 10.0) > 0.8, (np.sort(err)[:10], len(err))
    # and the recovered homography IS that mapping where it is supported by data: the corners of the bounding box of the
    # verified points in image 1 land where cat.txt sends them (the one reference-held anchor of the whole detect ->
    # describe -> match -> verify chain; the image corners themselves are an extrapolation of ~30 clustered matches of a
    # non-planar scene and move by hundreds of pixels)
    x0, y0, x1, y1 = p1[:, 0].min(), p1[:, 1].min(), p1[:, 0].max(), p1[:, 1].max()
    cor = np.array([[x0, y0, 1], [x1, y0, 1], [x1, y1, 1], [x0, y1, 1], [(x0 + x1) / 2, (y0 + y1) / 2, 1]], float)
    a = cor @ normH(got["H"]).T
    b = cor @ normH(Hgt).T
    cerr = np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1)
    print("cat support-box corners + centre vs cat.txt [px]:", np.round(cerr, 2), "box", np.round([x0, y0, x1, y1], 1))
    # measured: corners 7 .. 53 px, centre 9.5 px (the support is a 62 x 324 px strip, so H is loosely constrained across it)
    assert cerr[4] < CAT_CENTRE_TOL_PX and cerr[:4].max() < CAT_CORNER_TOL_PX, cerr


def test_match_fginn_full_size_multi_view_descriptors(ctx, modsx, oracle):
    """The distance kernels at the north-star size: the ~24 k x 24 k descriptors of a 1024x768 pair under the 31-view ladder
    (TiltSet 1,2,4,6,8, Phi 120) -- the same blob seen in 10-20 views, so most matched queries go through sweep 2 and the
    event kernel -- against the oracle's exact linear kNN + FGINN walk (OpenMP over the queries), every tentative field."""
    from mods_amd import synthetic
    a, b, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
    views = modsx.set_vs_pars([1.0], [1, 2, 4, 6, 8], 120.0, 0.2, 1, [])
    par = modsx.default_pair_params()
    ia, ib = ctx.upload(a), ctx.upload(b)
    r1, d1 = ctx.detect_describe_views(ia, views, par)
    r2, d2 = ctx.detect_describe_views(ib, views, par)
    ia.free(); ib.free()
    assert len(d1) > 20000 and len(d2) > 20000
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    got = ctx.match_fginn(d1, d2, pos2, 0.8, 30.0)
    ref = oracle.match_fginn(d1, d2, pos2, 0.8, 30.0)
    assert len(ref) > 10000 and len(got) == len(ref)
    for f in ref.dtype.names:
        assert np.array_equal(got[f], ref[f]), f


def test_view_shard_path_world1_rccl(ctx, modsx, small_pair):
    """The native RCCL path (csrc/engine_shard.hip) on one GPU: a world-size-1 communicator, ncclAllGather of the counts,
    the 328-byte row blocks and the matcher's result rows on device buffers -- must equal the unsharded library calls."""
    from mods_amd import distributed as D
    a, b, _ = small_pair
    comm = D.NativeComm([ctx])
    try:
        assert comm.describe()["ranks_seen_by_rccl"] == 1
        views = modsx.set_vs_pars([1.0], [1, 2, 3, 4], 360.0, 0.2, 1, [])
        par = modsx.default_pair_params(ransac_seed=4)
        ia, ib = ctx.upload(a), ctx.upload(b)
        ref1, refd1, c1 = ctx.detect_describe_views(ia, views, par, want_counts=True)
        ref2, refd2 = ctx.detect_describe_views(ib, views, par)
        r1, d1ptr, cnt = comm.detect_describe_views_sharded(0, ia, views, par)
        assert same_records(r1, ref1) and np.array_equal(cnt, c1)
        # the gathered descriptors live in HBM: match them against image 2's through the sharded matcher
        import torch
        d2 = torch.from_numpy(refd2.astype(np.uint8)).cuda()
        pos2 = np.stack([ref2["reproj_kp"]["x"], ref2["reproj_kp"]["y"]], 1)
        tent = comm.match_fginn_sharded(0, d1ptr, len(r1), d2.data_ptr(), len(ref2), pos2, 0.8, 30.0)
        reft = ctx.match_fginn(refd1, refd2, pos2, 0.8, 30.0)
        assert len(tent) == len(reft) > 10
        for f in reft.dtype.names:
            assert np.array_equal(tent[f], reft[f]), f
        got = comm.match_pair_views_sharded(0, ia, ib, views, par, owner=0)
        ref = ctx.match_pair_views(ia, ib, views, par)
        assert got["n_regions"] == ref["n_regions"] and got["n_verified"] == ref["n_verified"]
        for f in ref["tentatives"].dtype.names:
            assert np.array_equal(got["tentatives"][f], ref["tentatives"][f]), f
        assert np.array_equal(got["ransac_inlier"], ref["ransac_inlier"]) and np.array_equal(got["H"], ref["H"])
        assert comm.describe()["all_gather_calls_rank0"] >= 5
        ia.free(); ib.free()
    finally:
        comm.close()


def _oracle_ladder(oracle, a, b, steps, min_matches, seed, ori_mr=1.0, threads=1):
    """the cviu parameter set through tests/common.py's oracle-side loop"""
    return oracle_ladder(oracle, a, b, steps, min_matches, seed, ori=(ori_mr, 41, 1, 0.8), threads=threads)


@pytest.mark.parametrize("min_matches", [10, 10 ** 6])
def test_iteration_ladder_matches_oracle(ctx, modsx, oracle, small_pair, min_matches):
    """HessianAffine steps 4-6 of iters_mods_cviu.ini in miniature: the view sets of later steps are de-duplicated
    against earlier ones (SetVSPars prev_par), regions accumulate, and the loop stops at minMatches."""
    a, b, H = small_pair
    need_ref(oracle)
    prev_o, prev_m = [], []
    steps_o, steps_m = [], []
    for tilts, phi, ratio in (([1], 360.0, 0.8), ([1, 2], 360.0, 0.8), ([1, 2], 120.0, 0.85)):
        vo = oracle.set_vs_pars([1.0], tilts, phi, 0.2, 1, prev_o)
        vm = modsx.set_vs_pars([1.0], tilts, phi, 0.2, 1, prev_m)
        assert len(vo) == len(vm) and len(vo) > 0
        steps_o.append((vo, ratio)); steps_m.append((vm, ratio))
    ia, ib = ctx.upload(a), ctx.upload(b)
    got, done = ctx.match_ladder(ia, ib, steps_m, modsx.default_pair_params(ransac_seed=6), min_matches=min_matches)
    ia.free(); ib.free()
    ref, done_ref = _oracle_ladder(oracle, a, b, steps_o, min_matches, 6)
    assert done == done_ref and done == (1 if min_matches == 10 else 3)
    assert got["n_regions"] == ref["n_regions"] and got["n_tentatives"] == ref["n_tentatives"]
    for f in ref["tent"].dtype.names:
        assert np.array_equal(got["tentatives"][f], ref["tent"][f]), f
    assert np.array_equal(got["ransac_inlier"], ref["rr"]["inl"]) and np.array_equal(got["verified"], ref["rr"]["keep"])
    assert np.abs(normH(got["H"]) - normH(ref["rr"]["H"])).max() < 1e-4


def test_mser_device_path_and_view_loop(ctx, modsx, oracle, small_pair):
    """E1/E2 behind the device boundary: u8 truncation on the GPU, component tree on the host; then the MSER class of
    the per-view loop (synthesise, DetectMSERs, orient, reproject, describe) against the oracle-side loop."""
    a = small_pair[0]
    im = ctx.upload(a)
    got = ctx.detect_msers(im)
    ref = oracle.detect_msers(a)
    assert len(ref) > 100 and same_records(got, ref.view(modsx.KEYPOINT))
    vo, vm = _views(oracle, modsx, [1, 2], 360.0, sigma=0.8)
    mser_kw = dict(min_size=30, max_area=0.05, min_margin=8.0)
    par = modsx.default_pair_params(detector=3, ori_mrSize=5.1962)
    regs, desc = ctx.detect_describe_views(im, vm, par)
    r_ref, d_ref = oracle.detect_describe_views(a, vo, ori=(5.1962, 41, 1, 0.8), mser=mser_kw)
    im.free()
    assert len(r_ref) > 100 and len(regs) == len(r_ref)
    assert same_records(regs, r_ref.view(modsx.REGION)) and np.array_equal(desc, d_ref)
    assert set(np.unique(regs["type"])) == {3}


def test_mixed_mser_hessaff_ladder_matches_oracle(ctx, modsx, oracle, small_pair):
    """iters_mods_cviu.ini in miniature: an MSER step, then HessianAffine steps; the classes keep separate region lists
    and tentatives, the verified set comes from their concatenation (HessianAffine first)."""
    a, b, H = small_pair
    need_ref(oracle)
    prev_o, prev_m, steps_o, steps_m = {0: [], 3: []}, {0: [], 3: []}, [], []
    for det, tilts, phi, sigma, ratio in ((3, [1], 360.0, 0.8, 0.85), (0, [1], 360.0, 0.2, 0.8), (3, [1, 3], 360.0, 0.8, 0.8),
                                          (0, [1, 2], 360.0, 0.2, 0.8)):
        vo = oracle.set_vs_pars([1.0], tilts, phi, sigma, 1, prev_o[det])
        vm = modsx.set_vs_pars([1.0], tilts, phi, sigma, 1, prev_m[det])
        assert len(vo) == len(vm) and len(vo) > 0
        steps_o.append((vo, ratio, det)); steps_m.append((vm, ratio, det))
    ia, ib = ctx.upload(a), ctx.upload(b)
    got, done = ctx.match_ladder(ia, ib, steps_m, modsx.default_pair_params(ransac_seed=8), min_matches=10 ** 6)
    ia.free(); ib.free()
    ref, done_ref = _oracle_ladder(oracle, a, b, steps_o, 10 ** 6, 8)
    assert done == done_ref == 4
    assert got["n_regions"] == ref["n_regions"] and got["n_tentatives"] == ref["n_tentatives"]
    for f in ref["tent"].dtype.names:
        assert np.array_equal(got["tentatives"][f], ref["tent"][f]), f
    assert np.array_equal(got["ransac_inlier"], ref["rr"]["inl"]) and np.array_equal(got["verified"], ref["rr"]["keep"])
    assert np.abs(normH(got["H"]) - normH(ref["rr"]["H"])).max() < 1e-4
    assert np.abs(normH(got["H"]) - H).max() < 1.5


def test_flag_word_wait_path_gives_the_same_results():
    """MODSX_HOST_WAIT=flag (engine.hip: stage boundaries through the context's pinned flag word and small tables by copy kernels
    instead of hipStreamSynchronize / hipMemcpyAsync; `auto` takes it when the process is short of CPUs, so the default test process
    never runs it): Hessian-Affine and MSER view sets and a pair end to end against the oracle, twice on one context (the staging
    buffers and the flag's sequence numbers are reused), in a child process (the switch is read once per process); then the same
    with MODSX_HOST_WAIT=alternate, where calls take the two ways of waiting in turn."""
    import json, os, subprocess, sys
    code = (
        "import sys, json, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import mods_amd\n"
        "from mods_amd import synthetic\n"
        "from oracle import pyoracle as O\n"
        "from common import same_records, oracle_pair\n"
        "import os\n"
        "assert os.environ['MODSX_HOST_WAIT'] != 'flag' or mods_amd.lib().modsx_debug_host_wait_runtime() == 0\n"
        "a, b, _ = synthetic.make_pair(rows=240, cols=320, nblobs=420, seed=777)\n"
        "ctx = mods_amd.Context(0)\n"
        "ok = True\n"
        "vm = mods_amd.set_vs_pars([1.0], [1, 2, 3], 360.0, 0.2, 1, [])\n"
        "vo = O.set_vs_pars([1.0], [1, 2, 3], 360.0, 0.2, 1, [])\n"
        "rr, dd = O.detect_describe_views(a, vo)\n"
        "vm2 = mods_amd.set_vs_pars([1.0], [1, 2], 360.0, 0.8, 1, [])\n"
        "vo2 = O.set_vs_pars([1.0], [1, 2], 360.0, 0.8, 1, [])\n"
        "mr, md = O.detect_describe_views(a, vo2, ori=(5.1962, 41, 1, 0.8), mser=dict(min_size=30, max_area=0.05, min_margin=8.0))\n"
        "ref = oracle_pair(O, a, b, seed=3) if O.ref_available() else None\n"
        "n = 0\n"
        "for rep in range(2):\n"
        "    ia, ib = ctx.upload(a), ctx.upload(b)\n"
        "    r, d = ctx.detect_describe_views(ia, vm, mods_amd.default_pair_params())\n"
        "    ok = ok and same_records(r, rr.view(mods_amd.REGION)) and bool(np.array_equal(d, dd))\n"
        "    r2, d2 = ctx.detect_describe_views(ia, vm2, mods_amd.default_pair_params(detector=3, ori_mrSize=5.1962))\n"
        "    ok = ok and same_records(r2, mr.view(mods_amd.REGION)) and bool(np.array_equal(d2, md))\n"
        "    res = ctx.match_pair(ia, ib, mods_amd.default_pair_params(ransac_seed=3))\n"
        "    if ref is not None:\n"
        "        ok = ok and res['n_tentatives'] == len(ref['tent']) and bool(np.array_equal(res['ransac_inlier'], ref['ransac']['inl']))\n"
        "    n = len(r) + len(r2)\n"
        "    ia.free(); ib.free()\n"
        "print(json.dumps({'ok': bool(ok), 'n': int(n), 'verified': int(res['n_verified'])}))\n"
    ) % (ROOT, os.path.join(ROOT, "tests"))
    for mode in ("flag", "alternate"):      # alternate: every call latches the other mode (runtime <-> flag transitions, the drain)
        env = dict(os.environ, MODSX_HOST_WAIT=mode)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (mode, out.stderr[-2000:])
        res = json.loads(out.stdout.strip().splitlines()[-1])
        assert res["ok"] and res["n"] > 300 and res["verified"] > 20, mode


def _cviu_ladder(oracle, modsx):
    """[MSER2], [MSER3], [HessianAffine4..6] of build/iters_mods_cviu.ini: view sets of both sides, later steps de-duplicated
    against the earlier ones of their detector (SetVSPars prev_par)."""
    prev_o, prev_m, steps_o, steps_m = {0: [], 3: []}, {0: [], 3: []}, [], []
    for det, scales, tilts, phi, sigma, ratio in ((3, [1, 0.25, 0.125], [1], 360.0, 0.8, 0.85),
                                                 (3, [1, 0.25, 0.125], [1, 3, 6, 9], 360.0, 0.8, 0.8),
                                                 (0, [1], [1, 2, 4, 6, 8], 360.0, 0.2, 0.8),
                                                 (0, [1], [1, 2, 4, 6, 8], 120.0, 0.2, 0.8),
                                                 (0, [1], [1, 2, 4, 6, 8], 60.0, 0.2, 0.8)):
        vm = modsx.set_vs_pars(scales, tilts, phi, sigma, 1, prev_m[det])
        steps_m.append((vm, ratio, det))
        if oracle is not None:
            vo = oracle.set_vs_pars(scales, tilts, phi, sigma, 1, prev_o[det])
            assert len(vo) == len(vm) and len(vo) > 0
            steps_o.append((vo, ratio, det))
    return steps_o, steps_m


@pytest.mark.parametrize("ori_mr", [1.0, 5.1962])
def test_configs3_full_cviu_ladder_all_steps_matches_oracle(ctx, modsx, oracle, ori_mr):
    """configs[3] in its stated form on one GPU: the 1024x768 synthetic pair through ALL MSER and HessianAffine steps of
    iters_mods_cviu.ini (minMatches forced high): 27 MSER views and 61 HessianAffine views per image accumulate, every step
    re-matches its class; region counts, every tentative, the RANSAC inlier set, the verified set and H == the CPU oracle's
    loop (whose views run on a thread pool, as the reference's OpenMP loop does).  ori_mr 1.0 is [DominantOrientation] mrSize of
    config_iter_mods_cviu.ini:103 (the configuration the ladder ships with); 5.1962 is the WxBS file's value on the same ladder."""
    import os
    from mods_amd import synthetic
    need_ref(oracle)
    a, b, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
    steps_o, steps_m = _cviu_ladder(oracle, modsx)
    assert [len(v) for v, _, _ in steps_m] == [3, 24, 11, 20, 30]        # 27 MSER views, 61 HessianAffine views
    par = modsx.default_pair_params(ransac_seed=3, ori_mrSize=ori_mr)
    ia, ib = ctx.upload(a), ctx.upload(b)
    got, done = ctx.match_ladder(ia, ib, steps_m, par, min_matches=10 ** 6)
    ia.free(); ib.free()
    ref, done_ref = _oracle_ladder(oracle, a, b, steps_o, 10 ** 6, 3, ori_mr=ori_mr, threads=min(64, os.cpu_count() or 1))
    assert done == done_ref == 5
    assert got["n_regions"] == ref["n_regions"] and got["n_regions"][0] > 40000
    assert got["n_tentatives"] == ref["n_tentatives"] and len(ref["tent"]) > 5000
    for f in ref["tent"].dtype.names:
        assert np.array_equal(got["tentatives"][f], ref["tent"][f]), f
    assert np.array_equal(got["ransac_inlier"], ref["rr"]["inl"]) and np.array_equal(got["verified"], ref["rr"]["keep"])
    assert np.abs(normH(got["H"]) - normH(ref["rr"]["H"])).max() < 1e-4


WXBS_STEPS = (   # [MSER2], [MSER3], [HessianAffine4..6] of build/iters_mods_cviu_wxbs.ini:30-75: Descriptors=RootSIFT,HalfRootSIFT
    (3, [1, 0.25, 0.125], [1], 360.0, 0.8, [(1, 0.85), (3, 0.8)]),
    (3, [1, 0.25, 0.125], [1, 3, 6, 9], 360.0, 0.8, [(1, 0.8), (3, 0.8)]),
    (0, [1], [1, 2, 4, 6, 8], 360.0, 0.2, [(1, 0.8), (3, 0.8)]),
    (0, [1], [1, 2, 4, 6, 8], 120.0, 0.2, [(1, 0.8), (3, 0.8)]),
    (0, [1], [1, 2, 4, 6, 8], 60.0, 0.2, [(1, 0.9), (3, 0.9)]))


def _wxbs_ladder(oracle, modsx, which=None):
    prev_o, prev_m, steps_o, steps_m = {0: [], 3: []}, {0: [], 3: []}, [], []
    for i, (det, scales, tilts, phi, sigma, descs) in enumerate(WXBS_STEPS):
        vm = modsx.set_vs_pars(scales, tilts, phi, sigma, 1, prev_m[det])
        vo = oracle.set_vs_pars(scales, tilts, phi, sigma, 1, prev_o[det]) if oracle is not None else None
        if which is not None and i not in which:
            continue
        steps_m.append((vm, 0.0, det, descs))
        if oracle is not None:
            assert len(vo) == len(vm) and len(vo) > 0
            steps_o.append((vo, 0.0, det, descs))
    return steps_o, steps_m


def _wxbs_ladder_params(modsx, seed, useF, reg_number=2000, mser_regs=500):
    """config_iter_mods_cviu_wxbs.ini: [MSER] :4-12 (FixedRegNumber 500), [HessianAffine] :13-27 (NotLessThanRegions 2000),
    [DominantOrientation] :102-108, [SIFTDescriptor] :109-118, contradDist :173, [DuplicateFiltering] :179-182, [RANSAC] :185-194"""
    par = modsx.default_pair_params(
        mode=4, threshold=5.3333, reg_number=reg_number, ori_mrSize=5.1962, ori_maxAngles=5, ori_threshold=0.8,
        desc_mrSize=5.1962, desc_photoNorm=1, desc_maxBinValue=0.2, contradDist=10.0, duplicateDist=3.0,
        err_threshold=4.0, confidence=0.99, max_samples=1000000, localOptimization=1, LAFCoef=3.0, HLAFCoef=13.0,
        doSymmCheck=1, useF=useF, ransac_seed=seed)
    par.mser.mode = 2
    par.mser.reg_number = mser_regs
    return par


def _check_wxbs_ladder(oracle, modsx, ctx, a, b, steps_o, steps_m, useF, seed, min_matches, reg_number, mser_regs, threads=1):
    par = _wxbs_ladder_params(modsx, seed, useF, reg_number, mser_regs)
    ia, ib = ctx.upload(a), ctx.upload(b)
    got, done = ctx.match_ladder(ia, ib, steps_m, par, min_matches=min_matches)
    ia.free(); ib.free()
    rk = dict(kind="f", err_threshold=4.0, max_samples=1000000, laf_coef=3.0) if useF else \
        dict(kind="h", err_threshold=4.0, max_samples=1000000, hlaf_coef=13.0)
    ref, done_ref = oracle_ladder(oracle, a, b, steps_o, min_matches, seed, ori=(5.1962, 41, 5, 0.8), threads=threads,
                                  hess=oracle.default_params(mode=4, threshold=5.3333, reg_number=reg_number),
                                  mser_kw=dict(min_size=30, max_area=0.05, min_margin=8.0, mode=2, reg_number=mser_regs),
                                  contrad=10.0, dup_dist=3.0, ransac=rk)
    assert done == done_ref
    assert got["n_regions"] == ref["n_regions"] and got["n_tentatives"] == ref["n_tentatives"]
    for f in ref["tent"].dtype.names:
        assert np.array_equal(got["tentatives"][f], ref["tent"][f]), f
    assert np.array_equal(got["ransac_inlier"], ref["rr"]["inl"]) and np.array_equal(got["verified"], ref["rr"]["keep"])
    if useF:
        Fa, Fb = ref["rr"]["F"] / np.linalg.norm(ref["rr"]["F"]), got["H"] / np.linalg.norm(got["H"])
        if (Fa * Fb).sum() < 0:
            Fb = -Fb
        assert np.abs(Fa - Fb).max() < 1e-6
    else:
        assert np.abs(normH(got["H"]) - normH(ref["rr"]["H"])).max() < 1e-4
    return got, ref, done


@pytest.mark.parametrize("useF", [0, 1])
def test_wxbs_ladder_two_descriptor_classes_small(ctx, modsx, oracle, small_pair, useF):
    """The WxBS ladder (iters_mods_cviu_wxbs.ini [MSER2], [MSER3], [HessianAffine4..6]) in its stated form on a small pair: every
    step carries RootSIFT AND HalfRootSIFT, so it orients with the Half-folded histogram, keeps one region list and one
    tentative list per (detector, descriptor), matches each with its own FGINN threshold (0.85 / 0.8 in [MSER2], 0.9 in
    [HessianAffine6]) and verifies the concatenation in std::map order -- H (ver_type 0) and F (ver_type 2)."""
    a, b, H = small_pair
    need_ref(oracle)
    steps_o, steps_m = _wxbs_ladder(oracle, modsx)
    assert [len(v) for v, _, _, _ in steps_m] == [3, 24, 11, 20, 30]
    got, ref, done = _check_wxbs_ladder(oracle, modsx, ctx, a, b, steps_o, steps_m, useF, 7, 10 ** 6, 300, 120)
    assert done == 5 and got["n_verified"] > 30
    n1 = got["n_regions"][0]
    assert (got["tentatives"]["q"] < n1 // 2).any() and (got["tentatives"]["q"] >= n1 // 2).any()
    if not useF:
        assert np.abs(normH(got["H"]) - H).max() < 2.5
    # minMatches = 15 (iters_mods_cviu_wxbs.ini:3): the same ladder stops as soon as the verified set is large enough
    got2, ref2, done2 = _check_wxbs_ladder(oracle, modsx, ctx, a, b, steps_o, steps_m, useF, 7, 15, 300, 120)
    assert done2 < 5


def test_configs4_wxbs_ladder_full_size_both_classes(ctx, modsx, oracle):
    """configs[4]'s ladder at full size: [MSER2], [HessianAffine4], [HessianAffine5] of iters_mods_cviu_wxbs.ini on the 1024x768
    pair with the WxBS parameter set (3 MSER views, 31 HessianAffine views; two descriptor classes per detector = four
    classes), every tentative, the inlier set, the verified set and H against the oracle's loop."""
    import os
    from mods_amd import synthetic
    need_ref(oracle)
    a, b, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
    steps_o, steps_m = _wxbs_ladder(oracle, modsx, which=(0, 2, 3))
    assert [len(v) for v, _, _, _ in steps_m] == [3, 11, 20]
    got, ref, done = _check_wxbs_ladder(oracle, modsx, ctx, a, b, steps_o, steps_m, 0, 3, 10 ** 6, 2000, 500,
                                        threads=min(64, os.cpu_count() or 1))
    assert done == 3 and got["n_regions"][0] > 40000 and len(ref["tent"]) > 3000


def test_configs4_wxbs_ladder_full_size_remaining_steps(ctx, modsx, oracle):
    """The two steps of the WxBS ladder the test above leaves out, at 1024x768: [MSER3] (24 further MSER views: scales 1, 0.25,
    0.125 x tilts 3, 6, 9) and [HessianAffine6] (30 further views at Phi 60, FGINN 0.9), each on top of its detector's first
    step -- so all five steps of iters_mods_cviu_wxbs.ini meet the oracle at full size."""
    import os
    from mods_amd import synthetic
    need_ref(oracle)
    a, b, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
    th = min(64, os.cpu_count() or 1)
    for which, nviews in (((0, 1), [3, 24]), ((2, 4), [11, 30])):
        steps_o, steps_m = _wxbs_ladder(oracle, modsx, which=which)
        assert [len(v) for v, _, _, _ in steps_m] == nviews
        got, ref, done = _check_wxbs_ladder(oracle, modsx, ctx, a, b, steps_o, steps_m, 0, 3, 10 ** 6, 2000, 500, threads=th)
        assert done == 2 and len(ref["tent"]) > 300


def test_configs4_wxbs_ladder_1920x1080_identity_and_first_view_step(ctx, modsx, oracle):
    """configs[4]'s image size: a 1920x1080 pair of the batch generator (seeds 1000 / 2000) through
    [MSER2] (identity + two zooms) and [HessianAffine4] (11 views), H and F verification, against the oracle's loop."""
    import os
    from mods_amd import synthetic
    need_ref(oracle)
    a, b, _ = synthetic.make_pair(rows=1080, cols=1920, nblobs=4000, seed=1000)
    th = min(64, os.cpu_count() or 1)
    steps_o, steps_m = _wxbs_ladder(oracle, modsx, which=(0, 2))
    assert [len(v) for v, _, _, _ in steps_m] == [3, 11]
    for useF in (0, 1):
        got, ref, done = _check_wxbs_ladder(oracle, modsx, ctx, a, b, steps_o, steps_m, useF, 3, 10 ** 6, 2000, 500, threads=th)
        assert done == 2 and got["n_regions"][0] > 15000 and len(ref["tent"]) > 1000


def test_cat_pair_full_ladder_stops_early_on_ground_truth(ctx, modsx, cat_pair):
    """The HessianAffine / MSER part of build/iters_mods_cviu.ini on the reference's example pair: [MSER2] (scales 1,
    0.25, 0.125), [MSER3] (tilts 1, 3, 6, 9), [HessianAffine4..6] (tilts 1, 2, 4, 6, 8; phi 360, 120, 60), minMatches 10.
    The ladder must stop as soon as 10 verified correspondences exist and they must obey the shipped ground truth."""
    cat, cat2, Hgt = cat_pair
    i1, i2 = ctx.upload(cat), ctx.upload(cat2)
    prev = {0: [], 3: []}
    steps = []
    for det, scales, tilts, phi, sigma, ratio in ((3, [1, 0.25, 0.125], [1], 360.0, 0.8, 0.85),
                                                 (3, [1, 0.25, 0.125], [1, 3, 6, 9], 360.0, 0.8, 0.8),
                                                 (0, [1], [1, 2, 4, 6, 8], 360.0, 0.2, 0.8),
                                                 (0, [1], [1, 2, 4, 6, 8], 120.0, 0.2, 0.8),
                                                 (0, [1], [1, 2, 4, 6, 8], 60.0, 0.2, 0.8)):
        v = modsx.set_vs_pars(scales, tilts, phi, sigma, 1, prev[det])
        if v:
            steps.append((v, ratio, det))
    par = modsx.default_pair_params(ransac_seed=3, ori_mrSize=5.1962)
    got, done = ctx.match_ladder(i1, i2, steps, par, min_matches=10)
    full, done_full = ctx.match_ladder(i1, i2, steps[:done], par, min_matches=10 ** 6)
    i1.free(); i2.free()
    assert 1 <= done <= len(steps) and got["n_verified"] >= 10
    assert done_full == done and full["n_verified"] == got["n_verified"]          # deterministic, stops exactly there
    if done > 1:
        i1, i2 = ctx.upload(cat), ctx.upload(cat2)
        before, _ = ctx.match_ladder(i1, i2, steps[:done - 1], par, min_matches=10 ** 6)
        i1.free(); i2.free()
        assert before["n_verified"] < 10                                            # the previous step had not reached minMatches
    # the verified correspondences obey the shipped ground-truth homography (cat.txt): rebuild the concatenated region
    # lists (HessianAffine class first, then MSER, each in step order) the result indexes
    i1, i2 = ctx.upload(cat), ctx.upload(cat2)
    lists = {0: [[], []], 3: [[], []]}
    for v, _, det in steps[:done]:
        pd = modsx.default_pair_params(ransac_seed=3, ori_mrSize=5.1962, detector=det)
        for side, im in enumerate((i1, i2)):
            r, _ = ctx.detect_describe_views(im, v, pd, want_desc=False)
            lists[det][side].append(r)
    i1.free(); i2.free()
    r1 = np.concatenate([r for det in (0, 3) for r in lists[det][0]] or [np.zeros(0, modsx.REGION)])
    r2 = np.concatenate([r for det in (0, 3) for r in lists[det][1]] or [np.zeros(0, modsx.REGION)])
    assert got["n_regions"] == (len(r1), len(r2))
    t = got["tentatives"][got["verified"]]
    p1 = np.stack([r1["reproj_kp"]["x"][t["q"]], r1["reproj_kp"]["y"][t["q"]], np.ones(len(t))], 1)
    p2 = np.stack([r2["reproj_kp"]["x"][t["t0"]], r2["reproj_kp"]["y"][t["t0"]]], 1)
    proj = p1 @ normH(Hgt).T
    proj = proj[:, :2] / proj[:, 2:]
    err = np.linalg.norm(proj - p2, axis=1)
    # the scene is not exactly planar: the shipped H fits the matches to ~15 px
    assert np.mean(err < 10.0) > 0.6 and err.max() < 30.0, (done, np.sort(err)[-10:], len(err))


def test_match_pairs_views_equals_single_calls(modsx, small_pair):
    """modsx_match_pairs_views (contexts take pairs off a counter, verification on helper threads) returns what
    modsx_match_pair_views returns pair by pair."""
    a, b, _ = small_pair
    ctxs = [modsx.Context(0) for _ in range(3)]
    views = modsx.set_vs_pars([1.0], [1, 2, 3], 360.0, 0.2, 1, [])
    par = modsx.default_pair_params(ransac_seed=9)
    ims = [(ctxs[0].upload(a), ctxs[0].upload(b)), (ctxs[0].upload(b), ctxs[0].upload(a))]
    i1 = [ims[i % 2][0] for i in range(7)]
    i2 = [ims[i % 2][1] for i in range(7)]
    got = modsx.match_pairs_views(ctxs, i1, i2, views, par)
    check_batch_statistics(modsx, 3, 7, 1)
    light = modsx.match_pairs_views(ctxs, i1, i2, views, par, arrays=False)
    check_batch_statistics(modsx, 3, 7, 1)
    for i in range(7):
        ref = ctxs[0].match_pair_views(i1[i], i2[i], views, par)
        for k in ("n_regions", "n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples"):
            assert got[i][k] == ref[k] and light[i][k] == ref[k], k
        assert np.array_equal(got[i]["H"], ref["H"]) and np.array_equal(got[i]["verified"], ref["verified"])
        assert same_records(got[i]["tentatives"], ref["tentatives"])
    assert modsx.match_pairs_views(ctxs, [], [], views, par) == []
    for x, y in ims:
        x.free(); y.free()


def test_a_refused_pair_fails_the_whole_views_batch(modsx, small_pair):
    """Three pairs over two contexts with a view list whose second view the host planner refuses (views_plan.cpp, before any
    kernel of that view set is launched): the batch call raises the planner's error and returns nothing; the same contexts then
    run the good list and give what modsx_match_pair_views gives pair by pair."""
    a, b, _ = small_pair
    ctxs = [modsx.Context(0) for _ in range(2)]
    good = modsx.set_vs_pars([1.0], [1, 2, 3], 360.0, 0.2, 1, [])
    assert len(good) >= 2
    bad = list(good)
    bad[1] = modsx.make_view(1e9, 0.0, 1.0, 0.2, 1)
    with pytest.raises(RuntimeError, match="degenerate"):      # the refusal is the host's
        modsx.view_plan(a.shape[0], a.shape[1], bad[1])
    par = modsx.default_pair_params(ransac_seed=9)
    ia, ib = ctxs[0].upload(a), ctxs[0].upload(b)
    i1, i2 = [ia, ib, ia], [ib, ia, ib]
    with pytest.raises(RuntimeError, match="degenerate"):
        modsx.match_pairs_views(ctxs, i1, i2, bad, par)
    got = modsx.match_pairs_views(ctxs, i1, i2, good, par)
    check_batch_statistics(modsx, 2, 3, 1)
    for i in range(3):
        ref = ctxs[0].match_pair_views(i1[i], i2[i], good, par)
        for k in ("n_regions", "n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples"):
            assert got[i][k] == ref[k], k
        assert np.array_equal(got[i]["H"], ref["H"]) and np.array_equal(got[i]["verified"], ref["verified"])
        assert same_records(got[i]["tentatives"], ref["tentatives"])
    assert got[0]["n_verified"] > 50
    ia.free(); ib.free()
    for c in ctxs:
        c.close()

