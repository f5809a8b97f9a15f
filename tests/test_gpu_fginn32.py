"""GPU: the f32 FGINN matcher (MatchFlannFGINN on float rows of any width; kernels_fginn32.hip, engine_fginn32.hip) against
oracle.pyoracle.match_fginn, bit for bit: count, q / t0 / tj / t1 and the f64 fields as bit patterns.  The inputs come from
tests/fginn32_cases.py; tests/test_fginn32_cases_cpu.py proves on the CPU what they reach."""
import os

import numpy as np
import pytest

from common import laf_of, need_ref, normH
import fginn32_cases as FC

pytestmark = pytest.mark.gpu


def _dev(rows, offset=0):
    """the f32 rows in a torch buffer on the device, `offset` bytes into it: (keep-alive, device pointer)"""
    import torch
    rows = np.ascontiguousarray(rows, np.float32)
    buf = torch.zeros(rows.size * 4 + 64, dtype=torch.uint8, device="cuda")
    buf[offset:offset + rows.size * 4] = torch.from_numpy(rows.reshape(-1).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _ref(oracle, c, nn=50, n1=None, n2=None):
    q = c["q"] if n1 is None else c["q"][:n1]
    t, pos = (c["t"], c["pos"]) if n2 is None else (c["t"][:n2], c["pos"][:n2])
    return oracle.match_fginn(q, t, pos, c["ratio"], c["cd"], nn)


def _debug(ctx, c, nn=50, splits=0, n1=None, n2=None, **kw):
    q = c["q"] if n1 is None else c["q"][:n1]
    t, pos = (c["t"], c["pos"]) if n2 is None else (c["t"][:n2], c["pos"][:n2])
    return ctx.debug_match_fginn_f32(q, t, pos, c["ratio"], c["cd"], nn, splits=splits, **kw)


def _keys(oracle, c, k=4):
    """the oracle's k nearest as the matcher's keys: (f32 bit pattern << 32) | index, all ones where there is no train"""
    idx, dist = oracle.knn_linear(c["q"], c["t"], k)
    key = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint32).astype(np.uint64)
    key[idx < 0] = np.uint64(0xffffffffffffffff)
    return key


@pytest.mark.parametrize("dim", [4, 8, 36, 64, 128, 132, 144, 192, 200, 256])
def test_widths_from_the_host_and_from_unaligned_device_rows(modsx, oracle, ctx, dim):
    T = modsx.fginn32_geometry(257, 1000, dim)["tile"]
    n1, n2 = 257, 2 * T + 3
    c = FC.random_case(n1, n2, dim, 100 + dim)
    ref = _ref(oracle, c)
    assert 20 < len(ref) < n1
    FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], 50), ref)
    dq, dt = _dev(c["q"], 4), _dev(c["t"], 4)            # rows 4 bytes off every wider alignment
    assert dq[1] % 8 == 4 and dt[1] % 8 == 4
    FC.same_tents(ctx.match_fginn_f32_device(dq[1], n1, dt[1], n2, dim, c["pos"], c["ratio"], c["cd"], 50), ref)
    r = _debug(ctx, c)
    FC.same_tents(r["tentatives"], ref)
    g = r["geometry"]
    assert g == modsx.fginn32_geometry(n1, n2, dim) and g["DK"] >= dim and g["tile"] == T and g["tiles"] == 3
    assert np.array_equal(r["top4"], _keys(oracle, c))


@pytest.mark.parametrize("nn", [2, 4, 50])
def test_sizes_around_wavefront_workgroup_tile_and_split(modsx, oracle, ctx, nn):
    dim = 128
    T = modsx.fginn32_geometry(257, 1000, dim)["tile"]
    c = FC.random_case(257, 2 * T + 3, dim, 7, noise=0.9)
    for n2 in (2, 3, T - 1, T, T + 1, 2 * T + 3):
        ref = _ref(oracle, c, nn, n2=n2)
        tiles = (n2 + T - 1) // T
        for n1 in (1, 63, 64, 65, 256, 257):
            want = ref[ref["q"] < n1]
            for splits in sorted({1, 2, 3, tiles}):
                r = _debug(ctx, c, nn, splits, n1, n2)
                g = r["geometry"]
                assert g["tile"] == T and g["tiles"] == tiles and g["splits"] <= min(splits, tiles)
                assert g == modsx.fginn32_geometry(n1, n2, dim, splits)
                FC.same_tents(r["tentatives"], want)
            FC.same_tents(_debug(ctx, c, nn, 0, n1, n2)["tentatives"], want)
    assert len(_ref(oracle, c, nn)) > 20


@pytest.mark.parametrize("nn", [2, 4, 50])
def test_walk_cases_take_the_stage_they_claim(modsx, oracle, ctx, nn):
    c = FC.walk_case()
    ref = _ref(oracle, c, nn)
    ia, da = oracle.knn_linear(c["q"], c["t"], len(c["t"]))
    stage = FC.expected_stage(ia, da, c["pos"], c["ratio"], c["cd"], nn)
    T = modsx.fginn32_geometry(len(c["q"]), len(c["t"]), 128)["tile"]
    tiles = (len(c["t"]) + T - 1) // T
    assert tiles >= 4
    first = None
    for splits in (0, 1, 2, 3, tiles):
        r = _debug(ctx, c, nn, splits)
        FC.same_tents(r["tentatives"], ref)
        assert np.array_equal(r["stage"], stage), splits
        for q, name in c["expect"].items():
            assert r["stage"][q] == (FC.EXPECT_STAGE_NN50[name] if nn == 50 else 0), name
        assert r["resolve"] == int((stage >= 1).sum()) and r["by_count"] == int((stage == 2).sum()) and r["records"] == len(ref)
        assert r["flag"] == 0
        first = r if first is None else first
        assert np.array_equal(r["top4"], first["top4"]) and np.array_equal(r["stage"], first["stage"])      # identical for every S
        FC.same_tents(r["tentatives"], first["tentatives"])
    assert np.array_equal(first["top4"], _keys(oracle, c))
    FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], nn), ref)
    if nn == 50:
        # with the resolve sweep switched off, exactly the queries that need it lose their records
        r = _debug(ctx, c, nn, 0, stage_mask=1)
        assert np.array_equal(r["stage"] >= 1, stage >= 1)
        FC.same_tents(r["tentatives"], ref[stage[ref["q"]] == 0])
        assert len(r["tentatives"]) < len(ref)


@pytest.mark.parametrize("make", [FC.short_case, FC.tiny_case, FC.threshold_case, FC.subnormal_case])
def test_short_threshold_and_subnormal_cases(modsx, oracle, ctx, make):
    c = make()
    for nn in (2, 4, 50):
        ref = _ref(oracle, c, nn)
        for splits in (0, 1, 2):
            r = _debug(ctx, c, nn, splits)
            FC.same_tents(r["tentatives"], ref)
        assert np.array_equal(r["top4"], _keys(oracle, c))
        FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], nn), ref)
    if make is FC.short_case:
        assert _debug(ctx, c, 50)["stage"][0] == 1 and len(ref) == 0       # the resolve sweep finds nothing that ends the walk
    if make is FC.tiny_case:
        assert _debug(ctx, c, 50)["top4"][0, 3] == np.uint64(0xffffffffffffffff)
    if make is FC.threshold_case:
        assert sorted(ref["q"]) == [0, 1, 2] and list(ref["tj"] == ref["t1"]) == [True, True, False]
    if make is FC.subnormal_case:
        assert len(ref) > 10


@pytest.mark.parametrize("splits", [0, 1, 2, 3, 1 << 20])
def test_planted_ties_across_tile_and_split_edges(modsx, oracle, ctx, splits):
    n1, dim = 70, 128
    T = modsx.fginn32_geometry(n1, 1000, dim)["tile"]
    geo = modsx.fginn32_geometry(n1, FC.TIE_TILES * T - 2, dim, splits)
    c = FC.tie_case(geo, n1, dim)
    ref = _ref(oracle, c)
    r = _debug(ctx, c, 50, splits)
    assert r["geometry"] == geo
    FC.same_tents(r["tentatives"], ref)
    for qi, (a, b) in enumerate(c["pairs"]):
        k = r["top4"][qi]
        assert (int(k[0]) & 0xffffffff, int(k[1]) & 0xffffffff) == (a, b) and k[0] >> np.uint64(32) == k[1] >> np.uint64(32)
        rec = r["tentatives"][r["tentatives"]["q"] == qi][0]
        assert (rec["t0"], rec["t1"]) == (a, b)
    assert np.array_equal(r["top4"], _keys(oracle, c))


def test_integer_rows_agree_with_the_int8_matcher(modsx, oracle, ctx):
    """integer sums below 2^24 are exact in both"""
    c = FC.integer_case(300, 700, 13)
    ref = _ref(oracle, c)
    assert len(ref) > 50
    FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], 50), ref)
    FC.same_tents(ctx.match_fginn(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], 50), ref)


def test_production_size(modsx, oracle, ctx):
    """4 096 x 20 011 x 128 in production geometry: several tiles per split and several splits"""
    n1, n2, dim = 4096, 20011, 128
    c = FC.unit_case(n1, n2, dim, 21)
    ref = _ref(oracle, c)
    assert 500 < len(ref) < n1
    r = _debug(ctx, c)
    g = r["geometry"]
    assert g == modsx.fginn32_geometry(n1, n2, dim) and g["splits"] >= 4 and g["tiles_per_split"] >= 2 and g["workgroups"] == 16 * g["splits"]
    FC.same_tents(r["tentatives"], ref)
    dq, dt = _dev(c["q"]), _dev(c["t"])
    FC.same_tents(ctx.match_fginn_f32_device(dq[1], n1, dt[1], n2, dim, c["pos"], c["ratio"], c["cd"], 50), ref)


def test_refusals_leave_the_context_usable(modsx, oracle, ctx):
    c = FC.random_case(65, 130, 36, 3)
    q, t, pos = c["q"], c["t"], c["pos"]
    ok = _ref(oracle, c)
    dq, dt = _dev(q), _dev(t)

    def refused(fn):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+"):      # MODSX_ERR_ARG with a message
            fn()
        FC.same_tents(ctx.match_fginn_f32(q, t, pos), ok)           # the 65 x 130 case again

    for bad in (np.nan, np.inf, -np.inf, 1.1e17, -2e17):
        for side in (0, 1):
            rows = [q.copy(), t.copy()]
            rows[side][5, 7] = bad
            refused(lambda: ctx.match_fginn_f32(rows[0], rows[1], pos))
            db = _dev(rows[side])
            ptrs = (db[1], dt[1]) if side == 0 else (dq[1], db[1])
            refused(lambda: ctx.match_fginn_f32_device(ptrs[0], len(q), ptrs[1], len(t), 36, pos))
    edge = q.copy()
    edge[5, 7] = np.float32(9.9e16)                                 # inside the limit
    assert len(ctx.match_fginn_f32(edge, t, pos)) >= 0
    for dim in (6, 34, 2, 0, 260, 258):
        refused(lambda: ctx.match_fginn_f32(np.zeros((5, dim), np.float32), np.zeros((7, dim), np.float32), pos[:7]))
        refused(lambda: ctx.match_fginn_f32_device(dq[1], 5, dt[1], 7, dim, pos[:7]))
    for nn in (1, 257, 0, -3):
        refused(lambda: ctx.match_fginn_f32(q, t, pos, nn=nn))
        refused(lambda: ctx.match_fginn_f32_device(dq[1], len(q), dt[1], len(t), 36, pos, nn=nn))
    for ratio in (float("nan"), 1.0, 1.5, -1.0, float("inf")):
        refused(lambda: ctx.match_fginn_f32(q, t, pos, ratio=ratio))
        refused(lambda: ctx.match_fginn_f32_device(dq[1], len(q), dt[1], len(t), 36, pos, ratio=ratio))
    refused(lambda: ctx.match_fginn_f32_device(dq[1], 4, dt[1], 2000001, 36, pos))          # a size argument only
    refused(lambda: ctx.match_fginn_f32_device(dq[1], 2000001, dt[1], 4, 36, pos))
    refused(lambda: ctx.match_fginn_f32_device(dq[1] + 2, 4, dt[1], 8, 36, pos))            # not 4-byte aligned
    regs = np.zeros(len(q), modsx.REGION)
    refused(lambda: ctx.match_regions_f32(regs, q, regs, q, modsx.default_pair_params(match_ratio=1.0)))
    refused(lambda: ctx.debug_match_fginn_f32(q, t, pos, stage_mask=2))


def test_empty_sides_give_no_records(modsx, ctx):
    c = FC.random_case(65, 130, 36, 3)
    q, t, pos = c["q"], c["t"], c["pos"]
    e, ep = np.zeros((0, 36), np.float32), np.zeros((0, 2))
    assert len(ctx.match_fginn_f32(e, t, pos)) == 0
    assert len(ctx.match_fginn_f32(q, e, ep)) == 0
    assert len(ctx.match_fginn_f32(e, e, ep)) == 0
    assert len(ctx.match_fginn_f32_device(0, 0, _dev(t)[1], len(t), 36, pos)) == 0
    assert len(ctx.match_fginn_f32_device(_dev(q)[1], len(q), 0, 0, 36, ep)) == 0
    regs = np.zeros(len(q), modsx.REGION)
    for a, b in ((0, len(q)), (len(q), 0)):
        r = ctx.match_regions_f32(regs[:a], q[:a], regs[:b], q[:b], modsx.default_pair_params())
        assert r["n_regions"] == (a, b) and r["n_tentatives"] == 0 and r["n_unique"] == 0 and r["n_verified"] == 0
        assert (r["H"] == -1).all() and len(r["tentatives"]) == 0


def _planted_pair(modsx, n=600, dim=144, seed=5):
    """n regions per side: 400 of the second side are the first side's under a homography (descriptor + noise), the rest is clutter"""
    rs = np.random.RandomState(seed)
    H = np.array([[1.1, 0.05, 20], [-0.03, 0.95, -10], [1e-5, 2e-5, 1]])
    p1 = rs.uniform(20, 900, (n, 2))
    x = np.c_[p1, np.ones(n)] @ H.T
    p2 = x[:, :2] / x[:, 2:] + rs.normal(0, 0.5, (n, 2))
    d1 = rs.randn(n, dim).astype(np.float32)
    d2 = (d1 + 0.25 * rs.randn(n, dim)).astype(np.float32)
    d2[400:] = rs.randn(n - 400, dim)
    p2[400:] = rs.uniform(20, 900, (n - 400, 2))
    perm = rs.permutation(n)
    d2, p2 = d2[perm], p2[perm]
    regs = []
    for p, A in ((p1, np.eye(2)), (p2, H[:2, :2])):
        r = np.zeros(n, modsx.REGION)
        r["id"] = np.arange(n)
        for kp in ("reproj_kp", "det_kp"):
            r[kp]["x"], r[kp]["y"] = p[:, 0], p[:, 1]
            r[kp]["a11"], r[kp]["a12"], r[kp]["a21"], r[kp]["a22"] = A[0, 0], A[0, 1], A[1, 0], A[1, 1]
            r[kp]["s"] = 3
        regs.append(r)
    return regs[0], d1, regs[1], d2


def _pts(r1, r2, tent):
    return np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                     r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)


@pytest.mark.parametrize("use_f", [0, 1])
def test_fused_call_is_match_plus_duplicate_filter_plus_loransac(modsx, oracle, ctx, use_f):
    r1, d1, r2, d2 = _planted_pair(modsx)
    seed = 1
    par = modsx.default_pair_params(ransac_seed=seed, useF=1, LAFCoef=2.0, err_threshold=4.0) if use_f else \
        modsx.default_pair_params(ransac_seed=seed)
    got = ctx.match_regions_f32(r1, d1, r2, d2, par)
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    tent = ctx.match_fginn_f32(d1, d2, pos2, par.match_ratio, par.contradDist, par.nn)
    FC.same_tents(tent, oracle.match_fginn(d1, d2, pos2, par.match_ratio, par.contradDist, par.nn))
    assert len(tent) >= 300
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
        FC.same_tents(got["tentatives"], tu)
        assert np.array_equal(got["ransac_inlier"], rr["inl"]) and np.array_equal(got["verified"], rr["keep"])
        assert got["n_verified"] == rr["n"] and got["n_ransac_inliers"] == int(rr["inl"].sum())
        assert got["ransac_samples"] == rr["samples"]

    tu, rr = stages(modsx)
    same(tu, rr)
    assert np.array_equal(got["H"], rr["F"] if use_f else rr["H"])
    assert got["n_verified"] >= 200
    need_ref(oracle)
    tu, rr = stages(oracle)
    same(tu, rr)
    if use_f:
        Fa, Fb = rr["F"] / np.linalg.norm(rr["F"]), got["H"] / np.linalg.norm(got["H"])
        assert min(np.abs(Fa - Fb).max(), np.abs(Fa + Fb).max()) < 1e-6
    else:
        assert np.abs(normH(got["H"]) - normH(rr["H"])).max() < 1e-4


def test_key_file_round_trip(modsx, oracle, ctx, tmp_path):
    """a 144-wide float class written with save_regions, read with load_regions and matched: the result from the arrays.  The values
    are eighths below 125, exact in the key file's six significant digits and no integers: the 0..255 entries refuse them."""
    rs = np.random.RandomState(77)
    t = rs.randint(-999, 1000, (130, 144)).astype(np.float32) / 8
    q = t[rs.randint(0, 130, 65)] + rs.randint(-40, 41, (65, 144)).astype(np.float32) / 8
    pos = rs.uniform(0, 100, (130, 2))
    path = os.path.join(str(tmp_path), "liop.txt")
    loaded = []
    for rows in (q, t):
        r = np.zeros(len(rows), modsx.REGION)
        r["id"] = np.arange(len(r))
        r["reproj_kp"]["a11"] = r["reproj_kp"]["a22"] = r["det_kp"]["a11"] = r["det_kp"]["a22"] = 1
        r["reproj_kp"]["s"] = r["det_kp"]["s"] = 3
        modsx.save_regions(path, [("HessianAffine", "LIOP", r, rows, 144)])
        _, dn, lr, ld = modsx.load_regions(path, "HessianAffine", "LIOP")
        assert dn == "LIOP" and ld.shape == rows.shape and ld.dtype == np.float32 and len(lr) == len(r)
        assert np.array_equal(ld, rows)
        loaded.append(ld)
    ref = ctx.match_fginn_f32(q, t, pos)
    assert 10 < len(ref) <= len(q)
    FC.same_tents(ctx.match_fginn_f32(loaded[0], loaded[1], pos), ref)
    FC.same_tents(ref, oracle.match_fginn(q, t, pos))
    with pytest.raises(RuntimeError, match=r"\(-1\): .+"):
        ctx.match_fginn(np.tile(q[:, :128], 1), np.tile(t[:, :128], 1), pos)      # the int8 entry keeps its refusal
