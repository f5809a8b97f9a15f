"""GPU: the Hamming matcher (MatchFLANNDistance with the exact search; kernels_hamming.hip, engine_hamming.hip) against
tests/hamming_model.py, field-wise and exact.  The model is pinned to the oracle on the CPU (tests/test_hamming_model_cpu.py)."""
import os

import numpy as np
import pytest

from common import laf_of, need_ref, normH
import hamming_model as M

pytestmark = pytest.mark.gpu


def _dev(rows, offset=0):
    """the rows in a torch buffer on the device, `offset` bytes into it: (keep-alive, device pointer)"""
    import torch
    rows = np.ascontiguousarray(rows, np.uint8)
    buf = torch.zeros(rows.size + 32, dtype=torch.uint8, device="cuda")
    buf[offset:offset + rows.size] = torch.from_numpy(rows.reshape(-1)).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _search(ctx, q, t, splits=0, n1=None, n2=None, dev=None):
    (kq, pq), (kt, pt) = dev if dev is not None else (_dev(q), _dev(t))
    return ctx.debug_match_hamming(pq, len(q) if n1 is None else n1, pt, len(t) if n2 is None else n2, q.shape[1], splits)


def _small_case(nbytes):
    return M.random_rows(65, 130, nbytes, 100 + nbytes)


@pytest.mark.parametrize("nbytes", [1, 3, 4, 5, 16, 31, 32, 33, 61, 64])
def test_widths_host_u8_host_f32_and_device_agree_with_the_model(modsx, ctx, nbytes):
    q, t = _small_case(nbytes)
    nn2 = M.knn2(q, t)
    thr_mid = float(np.median(nn2[:, 1]))
    odd = nbytes % 2
    dq, dt = _dev(q, odd), _dev(t, odd)       # odd widths: rows one byte off every alignment
    assert not odd or (dq[1] % 2 == 1 and dt[1] % 2 == 1)
    raw, geo = ctx.debug_match_hamming(dq[1], len(q), dt[1], len(t), nbytes)
    assert np.array_equal(raw, nn2)
    assert geo == modsx.hamming_geometry(len(q), len(t), nbytes) and geo["W"] == (nbytes + 3) // 4
    for thr in (1e9, max(thr_mid, 0.5)):
        ref = M.tentatives(nn2, thr)
        assert 0 < len(ref) <= len(q)
        M.same_tents(ctx.match_hamming(q, t, thr), ref)
        M.same_tents(ctx.match_hamming(q.astype(np.float32), t.astype(np.float32), thr), ref)
        M.same_tents(ctx.match_hamming_device(dq[1], len(q), dt[1], len(t), nbytes, thr), ref)


@pytest.mark.parametrize("nbytes", [32, 5])
def test_tile_and_split_boundaries(modsx, ctx, nbytes):
    """n2 around the tile length, n1 around the wavefront and the workgroup, every split count: the raw search result is the
    model's whatever the geometry"""
    T = _search(ctx, *M.random_rows(4, 8, nbytes, 1))[1]["tile"]
    assert T == modsx.hamming_geometry(4, 8, nbytes)["tile"]
    q, t = M.random_rows(257, 2 * T + 1, nbytes, 7)
    dev = (_dev(q), _dev(t))
    for n2 in (2, 3, T - 1, T, T + 1, 2 * T + 1):
        ref = M.knn2(q, t[:n2])
        smax = modsx.hamming_geometry(257, n2, nbytes, 1 << 20)["splits"]
        assert smax == (n2 + T - 1) // T
        for n1 in (1, 63, 64, 65, 255, 256, 257):
            for splits in sorted({1, 2, 3, 7, smax}):
                got, geo = _search(ctx, q, t, splits, n1, n2, dev)
                assert geo["tile"] == T and geo["splits"] == min(splits, smax) and geo["workgroups"] == geo["splits"] * ((n1 + 255) // 256)
                assert np.array_equal(got, ref[:n1]), (n2, n1, splits)
            got, geo = _search(ctx, q, t, 0, n1, n2, dev)
            assert np.array_equal(got, ref[:n1]), (n2, n1, "production")


def test_tie_heavy_case_is_the_same_under_every_split_count(modsx, ctx):
    q, t = M.tie_heavy()
    ref = M.knn2(q, t)
    for splits in (0, 1, 2, 3, 7):
        assert np.array_equal(_search(ctx, q, t, splits)[0], ref)
    # the same rows nine times over: three tiles of 4-byte rows, so that the split counts differ in more than name
    t9 = np.tile(t, (9, 1))
    ref9 = M.knn2(q, t9)
    assert (ref9[:, 1] == ref9[:, 3]).all()
    dev = (_dev(q), _dev(t9))
    used = set()
    for splits in (0, 1, 2, 3, 7):
        got, geo = _search(ctx, q, t9, splits, dev=dev)
        used.add(geo["splits"])
        assert np.array_equal(got, ref9), splits
    assert used == {1, 2, 3}
    M.same_tents(ctx.match_hamming(q, t9, 4), M.tentatives(ref9, 4))


def test_planted_ties_across_tiles_and_splits(modsx, ctx):
    """a query's nearest train stands at index 0, at the last index of the first tile and at the first index of the last split: the
    two lowest indices win, for the first and for the second neighbour"""
    nbytes, n1 = 32, 300
    T = modsx.hamming_geometry(n1, 1000, nbytes)["tile"]
    n2 = 5 * T + 3
    for splits in (1, 2, 3, 7, 1 << 20, 0):
        g = modsx.hamming_geometry(n1, n2, nbytes, splits)
        start = M.last_split_start(T, n2, g["splits"])
        copies = M.copies_for(T, start) if g["splits"] > 1 else [0, T - 1, T]
        q, t, info = M.planted(n1, n2, nbytes, copies)
        got, geo = _search(ctx, q, t, splits)
        assert geo == g
        M.check_planted(got, info)
        assert tuple(got[M.PLANT["copies"]]) == (0, 2, T - 1, 2)
        assert np.array_equal(got, M.knn2(q, t))


def test_thresholds(modsx, ctx):
    q, t, _ = M.planted(300, 643, 32, [0, 127, 512])
    nn2 = M.knn2(q, t)
    counts = []
    for thr in (60, 60.9, 0.5, 1e9):
        ref = M.tentatives(nn2, thr)
        got = ctx.match_hamming(q, t, thr)
        M.same_tents(got, ref)
        counts.append(len(got))
    assert counts[0] == counts[1] and 0 < counts[2] < counts[0] < counts[3] == len(q)
    got = ctx.match_hamming(q, t, 60)
    assert np.isnan(got["ratio"][got["q"] == M.PLANT["nan"]]).all() and M.PLANT["at_max"] in got["q"] and M.PLANT["above_max"] not in got["q"]


def test_one_larger_problem_in_production_geometry(modsx, ctx):
    """8 192 x 20 011 rows of 32 bytes: several tiles per split and several splits"""
    n1, n2, nbytes = 8192, 20011, 32
    rs = np.random.RandomState(21)
    t = rs.randint(0, 256, (n2, nbytes)).astype(np.uint8)
    q = t[rs.randint(0, n2, n1)] ^ np.packbits(rs.rand(n1, 8 * nbytes) < rs.uniform(0, 0.5, (n1, 1)), axis=1)
    ref = M.knn2(q, t)
    got, geo = _search(ctx, q, t)
    ntiles = (n2 + geo["tile"] - 1) // geo["tile"]
    assert geo["splits"] >= 4 and ntiles > 2 * geo["splits"] and geo["workgroups"] == 32 * geo["splits"]
    assert np.array_equal(got, ref)
    tent = ctx.match_hamming(q, t, 60)
    assert 1000 < len(tent) < n1
    M.same_tents(tent, M.tentatives(ref, 60))


def test_refusals_leave_the_context_usable(modsx, ctx):
    q, t = _small_case(16)
    ok = M.match(q, t, 1e9)

    def refused(fn):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+"):      # MODSX_ERR_ARG with a message
            fn()
        M.same_tents(ctx.match_hamming(q, t, 1e9), ok)              # the 65 x 130 case again

    dq, dt = _dev(q), _dev(t)
    refused(lambda: ctx.match_hamming(q, t[:1], 60))                                          # n2 == 1
    refused(lambda: ctx.match_hamming(q[:0], t[:1], 60))
    refused(lambda: ctx.match_hamming_device(dq[1], len(q), dt[1], 1, 16, 60))
    refused(lambda: ctx.debug_match_hamming(dq[1], len(q), dt[1], 1, 16))
    refused(lambda: ctx.match_hamming(np.zeros((5, 0), np.uint8), np.zeros((7, 0), np.uint8), 60))     # nbytes 0
    refused(lambda: ctx.match_hamming(np.zeros((5, 65), np.uint8), np.zeros((7, 65), np.uint8), 60))   # nbytes 65
    refused(lambda: ctx.match_hamming_device(dq[1], 4, dt[1], 8, 0, 60))
    refused(lambda: ctx.match_hamming_device(dq[1], 4, dt[1], 8, 65, 60))
    f = q.astype(np.float32)
    f[3, 2] += 0.5
    refused(lambda: ctx.match_hamming(f, t.astype(np.float32), 60))                           # a fractional f32 value
    f[3, 2] = 256
    refused(lambda: ctx.match_hamming(f, t.astype(np.float32), 60))
    f[3, 2] = np.nan
    refused(lambda: ctx.match_hamming(t.astype(np.float32), f, 60))
    for thr in (0, -1, float("nan"), float("inf")):
        refused(lambda: ctx.match_hamming(q, t, thr))
        refused(lambda: ctx.match_hamming_device(dq[1], len(q), dt[1], len(t), 16, thr))
    regs = np.zeros(len(q), modsx.REGION)
    refused(lambda: ctx.match_regions_hamming(regs, q, regs[:1], t[:1], 60, modsx.default_pair_params()))


def test_empty_sides_give_no_records(modsx, ctx):
    q, t = _small_case(16)
    e = np.zeros((0, 16), np.uint8)
    assert len(ctx.match_hamming(e, t, 60)) == 0
    assert len(ctx.match_hamming(q, e, 60)) == 0
    assert len(ctx.match_hamming(e, e, 60)) == 0
    assert len(ctx.match_hamming_device(0, 0, _dev(t)[1], len(t), 16, 60)) == 0
    regs = np.zeros(len(q), modsx.REGION)
    for a, b in ((0, len(q)), (len(q), 0)):
        r = ctx.match_regions_hamming(regs[:a], q[:a], regs[:b], q[:b], 60, modsx.default_pair_params())
        assert r["n_regions"] == (a, b) and r["n_tentatives"] == 0 and r["n_unique"] == 0 and r["n_verified"] == 0
        assert (r["H"] == -1).all() and len(r["tentatives"]) == 0


def _pts(r1, r2, tent):
    return np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                     r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)


@pytest.mark.parametrize("use_f", [0, 1])
def test_fused_call_is_match_plus_duplicate_filter_plus_loransac(modsx, oracle, ctx, small_pair, use_f):
    a, b, _ = small_pair
    seed = 1
    par = modsx.default_pair_params(ransac_seed=seed, useF=1, LAFCoef=2.0, err_threshold=4.0) if use_f else \
        modsx.default_pair_params(ransac_seed=seed)
    ia, ib = ctx.upload(a), ctx.upload(b)
    view = [modsx.make_view()]
    r1, d1 = ctx.detect_describe_views(ia, view, par)
    r2, d2 = ctx.detect_describe_views(ib, view, par)
    ia.free(); ib.free()
    b1, b2 = M.binarise(d1), M.binarise(d2)
    got = ctx.match_regions_hamming(r1, b1, r2, b2, 30, par)
    tent = ctx.match_hamming(b1, b2, 30)
    M.same_tents(tent, M.match(b1, b2, 30))
    assert not np.isnan(tent["ratio"]).any() and len(tent) >= 100
    pts = _pts(r1, r2, tent)

    def stages(lib):
        order, keep = lib.duplicate_filtering(pts, tent["ratio"], par.duplicateDist, True)
        sel = order[keep]
        tu, pu = tent[sel], pts[sel]
        l1, l2 = laf_of(r1, tu["q"]), laf_of(r2, tu["t0"])
        if use_f:
            rr = lib.loransac_f(pu, l1, l2, err_threshold=par.err_threshold, confidence=par.confidence, max_samples=par.max_samples,
                                lo=par.localOptimization, laf_coef=par.LAFCoef, sym_check=par.doSymmCheck, error_type=par.errorType,
                                seed=seed)
        else:
            rr = lib.loransac_h(pu, l1, l2, err_threshold=par.err_threshold, confidence=par.confidence, max_samples=par.max_samples,
                                lo=par.localOptimization, hlaf_coef=par.HLAFCoef, sym_check=par.doSymmCheck, seed=seed,
                                error_type=par.errorType)
        return tu, rr

    def same(tu, rr):
        assert got["n_regions"] == (len(r1), len(r2)) and got["n_tentatives"] == len(tent) and got["n_unique"] == len(tu)
        M.same_tents(got["tentatives"], tu)
        assert np.array_equal(got["ransac_inlier"], rr["inl"]) and np.array_equal(got["verified"], rr["keep"])
        assert got["n_verified"] == rr["n"] and got["n_ransac_inliers"] == int(rr["inl"].sum())
        assert got["ransac_samples"] == rr["samples"]

    tu, rr = stages(modsx)
    same(tu, rr)
    assert np.array_equal(got["H"], rr["F"] if use_f else rr["H"])
    assert got["n_verified"] >= 50
    need_ref(oracle)
    tu, rr = stages(oracle)
    same(tu, rr)
    if use_f:
        Fa, Fb = rr["F"] / np.linalg.norm(rr["F"]), got["H"] / np.linalg.norm(got["H"])
        assert min(np.abs(Fa - Fb).max(), np.abs(Fa + Fb).max()) < 1e-6
    else:
        assert np.abs(normH(got["H"]) - normH(rr["H"])).max() < 1e-4


def test_key_file_round_trip(modsx, ctx, tmp_path):
    q, t = M.random_rows(65, 130, 32, 77)
    path = os.path.join(str(tmp_path), "orb.txt")
    regs = [np.zeros(len(x), modsx.REGION) for x in (q, t)]
    loaded = []
    for r, rows in zip(regs, (q, t)):
        r["id"] = np.arange(len(r))
        r["reproj_kp"]["a11"] = r["reproj_kp"]["a22"] = r["det_kp"]["a11"] = r["det_kp"]["a22"] = 1
        r["reproj_kp"]["s"] = r["det_kp"]["s"] = 3
        modsx.save_regions(path, [("ORB", "ORB", r, rows.astype(np.float32), 32)])
        _, dn, lr, ld = modsx.load_regions(path, "ORB", "ORB")
        assert dn == "ORB" and ld.shape == rows.shape and ld.dtype == np.float32 and len(lr) == len(r)
        loaded.append(ld)
    nn2 = M.knn2(q, t)
    thr = float(np.median(nn2[:, 1]))
    ref = ctx.match_hamming(q, t, thr)
    assert 0 < len(ref) < len(q)
    M.same_tents(ctx.match_hamming(loaded[0], loaded[1], thr), ref)
    M.same_tents(ref, M.tentatives(nn2, thr))
