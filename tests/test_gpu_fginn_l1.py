"""GPU: FGINN matching under vector_dist = L1 -- the f32 search with MODSX_DIST_L1 (kernels_fginn32.hip) and the byte-row search of
the SIFT family (kernels_fginn_l1.hip) -- against the numpy model of tests/fginn_l1_model.py, bit for bit: count, q / t0 / tj / t1
and the f64 fields as bit patterns.  The inputs come from tests/fginn_l1_cases.py; tests/test_fginn_l1_model_cpu.py pins the model to
the oracle and proves on the CPU what the inputs reach."""
import numpy as np
import pytest

from common import laf_of
import fginn32_cases as FC
import fginn_l1_cases as LC
import fginn_l1_model as LM

pytestmark = pytest.mark.gpu

NONE = np.uint64(0xffffffffffffffff)


def _dev(rows, dtype, offset):
    """the rows in a torch buffer on the device, `offset` bytes into it: (keep-alive, device pointer)"""
    import torch
    raw = np.ascontiguousarray(rows, dtype).reshape(-1).view(np.uint8)
    buf = torch.zeros(raw.size + 64, dtype=torch.uint8, device="cuda")
    buf[offset:offset + raw.size] = torch.from_numpy(raw.copy()).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _keys(idx, dist):
    key = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint32).astype(np.uint64)
    key[idx < 0] = NONE
    return key


def _sub(c, n1=None, n2=None):
    q = c["q"] if n1 is None else c["q"][:n1]
    t, pos = (c["t"], c["pos"]) if n2 is None else (c["t"][:n2], c["pos"][:n2])
    return q, t, pos


def _f32(ctx, modsx, c, nn=50, splits=0, n1=None, n2=None, **kw):
    q, t, pos = _sub(c, n1, n2)
    return ctx.debug_match_fginn_f32(q, t, pos, c["ratio"], c["cd"], nn, splits=splits, dist=modsx.DIST_L1, **kw)


def _u8(ctx, c, nn=50, splits=0, n1=None, n2=None, **kw):
    q, t, pos = _sub(c, n1, n2)
    return ctx.debug_match_fginn_l1(q, t, pos, c["ratio"], c["cd"], nn, splits=splits, **kw)


N1S = (1, 63, 64, 65, 255, 256, 257)


# ---- the f32 search with the L1 chain ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 36, 64, 128, 144, 200, 256])
def test_f32_l1_sizes_splits_and_row_sources(modsx, ctx, dim):
    """one width per kernel width and both chunked ones; n1 around wavefront and workgroup, n2 around the tile, forced and
    production splits, nn = 2, 4, 50; rows from the host and device rows 4 bytes off every wider alignment"""
    T = modsx.fginn32_geometry(257, 1000, dim)["tile"]
    c = FC.random_case(257, 2 * T + 1, dim, 300 + dim, noise=0.9 if dim >= 36 else 0.3)
    records = 0
    for n2 in (1, 3, 4, T - 1, T, T + 1, 2 * T + 1):
        tiles = (n2 + T - 1) // T
        dq, dt = _dev(c["q"], np.float32, 4), _dev(c["t"][:n2], np.float32, 4)
        assert dq[1] % 8 == 4 and dt[1] % 8 == 4
        for nn in (2, 4, 50):
            ref = LM.match(c, nn, "l1", n2=n2)
            records += len(ref)
            for n1 in N1S:
                want = ref[ref["q"] < n1]
                for splits in (1, 2, 3, 0):
                    r = _f32(ctx, modsx, c, nn, splits, n1, n2)
                    g = r["geometry"]
                    assert g == modsx.fginn32_geometry(n1, n2, dim, splits) and g["tile"] == T and g["tiles"] == tiles
                    FC.same_tents(r["tentatives"], want)
                FC.same_tents(ctx.match_fginn_f32_device(dq[1], n1, dt[1], n2, dim, c["pos"][:n2], c["ratio"], c["cd"], nn,
                                                         dist=modsx.DIST_L1), want)
        idx, dist = LM.knn(c["q"], c["t"][:n2], 4, "l1")
        assert np.array_equal(_f32(ctx, modsx, c, 50, 0, None, n2)["top4"], _keys(idx, dist))
    assert records > 100
    FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], 50, dist=modsx.DIST_L1), LM.match(c, 50, "l1"))


@pytest.mark.parametrize("nn", [2, 4, 50])
def test_f32_l1_walk_cases_take_the_stage_they_claim(modsx, ctx, nn):
    c = LC.walk_case()
    ref = LM.match(c, nn, "l1")
    ia, da = LM.knn(c["q"], c["t"], len(c["t"]), "l1")
    stage = FC.expected_stage(ia, da, c["pos"], c["ratio"], c["cd"], nn)
    T = modsx.fginn32_geometry(len(c["q"]), len(c["t"]), 128)["tile"]
    tiles = (len(c["t"]) + T - 1) // T
    assert tiles >= 4
    for splits in (0, 1, 2, 3, tiles):
        r = _f32(ctx, modsx, c, nn, splits)
        FC.same_tents(r["tentatives"], ref)
        assert np.array_equal(r["stage"], stage), splits
        for q, name in c["expect"].items():
            assert r["stage"][q] == (LC.EXPECT_STAGE_NN50[name] if nn == 50 else 0), name
        assert r["resolve"] == int((stage >= 1).sum()) and r["by_count"] == int((stage == 2).sum()) and r["records"] == len(ref)
        assert r["flag"] == 0
        assert np.array_equal(r["top4"], _keys(ia[:, :4], da[:, :4]))
    if nn == 50:
        r = _f32(ctx, modsx, c, nn, 0, stage_mask=1)          # without the resolve sweep exactly the queries that need it lose
        FC.same_tents(r["tentatives"], ref[stage[ref["q"]] == 0])
        assert len(r["tentatives"]) < len(ref)


@pytest.mark.parametrize("make", [LC.threshold_case, LC.subnormal_case])
def test_f32_l1_threshold_and_subnormal_cases(modsx, ctx, make):
    c = make()
    for nn in (2, 4, 50):
        ref = LM.match(c, nn, "l1")
        for splits in (0, 1, 2):
            FC.same_tents(_f32(ctx, modsx, c, nn, splits)["tentatives"], ref)
        FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], nn, dist=modsx.DIST_L1), ref)
    idx, dist = LM.knn(c["q"], c["t"], 4, "l1")
    r = _f32(ctx, modsx, c, 50)
    assert np.array_equal(r["top4"], _keys(idx, dist))
    if make is LC.threshold_case:
        assert sorted(ref["q"]) == [0, 1, 2] and list(ref["tj"] == ref["t1"]) == [True, True, False]
    else:
        assert len(ref) > 10 and (r["top4"][:, 1] >> np.uint64(32) > 0).all() and (r["top4"][:, 3] >> np.uint64(32) < 0x00800000).all()


@pytest.mark.parametrize("splits", [0, 1, 2, 3, 1 << 20])
def test_f32_l1_planted_ties_across_tile_and_split_edges(modsx, ctx, splits):
    n1, dim = 70, 128
    T = modsx.fginn32_geometry(n1, 1000, dim)["tile"]
    geo = modsx.fginn32_geometry(n1, LC.TIE_TILES * T - 2, dim, splits)
    c = LC.tie_case(geo, n1, dim)
    r = _f32(ctx, modsx, c, 50, splits)
    assert r["geometry"] == geo
    FC.same_tents(r["tentatives"], LM.match(c, 50, "l1"))
    for qi, (a, b) in enumerate(c["pairs"]):
        k = r["top4"][qi]
        assert (int(k[0]) & 0xffffffff, int(k[1]) & 0xffffffff) == (a, b) and k[0] >> np.uint64(32) == k[1] >> np.uint64(32)


def test_l2_through_the_new_entries_is_the_old_entries(modsx, oracle, ctx):
    c = FC.random_case(257, 99, 144, 41)
    q, t, pos = c["q"], c["t"], c["pos"]
    L, C = modsx.lib(), __import__("ctypes")
    ref = oracle.match_fginn(q, t, pos, c["ratio"], c["cd"], 50)
    old = ctx.match_fginn_f32(q, t, pos)
    FC.same_tents(old, ref)
    out = C.c_void_p()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    n = L.modsx_match_fginn_f32_dist(ctx.h, P(q), len(q), P(t), len(t), 144, P(pos), C.c_double(c["ratio"]), C.c_double(c["cd"]), 50,
                                     modsx.DIST_L2, C.byref(out))
    FC.same_tents(modsx._take(out, n, modsx.TENT), old)
    dq, dt = _dev(q, np.float32, 0), _dev(t, np.float32, 0)
    n = L.modsx_match_fginn_f32_dist_device(ctx.h, C.c_void_p(dq[1]), len(q), C.c_void_p(dt[1]), len(t), 144, P(pos), C.c_double(c["ratio"]),
                                            C.c_double(c["cd"]), 50, modsx.DIST_L2, C.byref(out))
    FC.same_tents(modsx._take(out, n, modsx.TENT), old)
    assert len(LM.match(c, 50, "l1")) > 10
    with pytest.raises(AssertionError):
        FC.same_tents(ctx.match_fginn_f32(q, t, pos, dist=modsx.DIST_L1), old)       # and L1 is another result


def _refused(ctx, fn, check):
    with pytest.raises(RuntimeError, match=r"\(-1\): .+"):      # MODSX_ERR_ARG with a message
        fn()
    check()


def test_f32_l1_refusals_leave_the_context_usable(modsx, ctx):
    c = FC.random_case(65, 130, 36, 3)
    q, t, pos = c["q"], c["t"], c["pos"]
    ok = LM.match(c, 50, "l1")
    L1 = modsx.DIST_L1
    dq, dt = _dev(q, np.float32, 0), _dev(t, np.float32, 0)
    again = lambda: FC.same_tents(ctx.match_fginn_f32(q, t, pos, dist=L1), ok)
    for bad in (np.nan, np.inf, 1.1e17):
        for side in (0, 1):
            rows = [q.copy(), t.copy()]
            rows[side][5, 7] = bad
            _refused(ctx, lambda: ctx.match_fginn_f32(rows[0], rows[1], pos, dist=L1), again)
            db = _dev(rows[side], np.float32, 0)
            ptrs = (db[1], dt[1]) if side == 0 else (dq[1], db[1])
            _refused(ctx, lambda: ctx.match_fginn_f32_device(ptrs[0], len(q), ptrs[1], len(t), 36, pos, dist=L1), again)
    for dim in (6, 34, 2, 0, 260):
        _refused(ctx, lambda: ctx.match_fginn_f32(np.zeros((5, dim), np.float32), np.zeros((7, dim), np.float32), pos[:7], dist=L1), again)
        _refused(ctx, lambda: ctx.match_fginn_f32_device(dq[1], 5, dt[1], 7, dim, pos[:7], dist=L1), again)
    for ratio in (float("nan"), 1.0, 1.5, -1.0):
        _refused(ctx, lambda: ctx.match_fginn_f32(q, t, pos, ratio=ratio, dist=L1), again)
        _refused(ctx, lambda: ctx.match_fginn_f32_device(dq[1], len(q), dt[1], len(t), 36, pos, ratio=ratio, dist=L1), again)
    regs = np.zeros(len(q), modsx.REGION)
    for dist in (2, -1, 100):
        _refused(ctx, lambda: ctx.match_fginn_f32(q, t, pos, dist=dist), again)
        _refused(ctx, lambda: ctx.match_fginn_f32_device(dq[1], len(q), dt[1], len(t), 36, pos, dist=dist), again)
        _refused(ctx, lambda: ctx.debug_match_fginn_f32(q, t, pos, dist=dist), again)
        _refused(ctx, lambda: ctx.match_regions_f32(regs, q, regs, q, modsx.default_pair_params(), dist=dist), again)
    _refused(ctx, lambda: ctx.match_regions_f32(regs, q, regs, q, modsx.default_pair_params(match_ratio=1.0), dist=L1), again)


# ---- the byte-row search ---------------------------------------------------------------------------------------------------
def test_u8_sizes_splits_and_row_sources(modsx, ctx):
    """the grid of the f32 test around the byte search's own tile length; rows from the host (f32 holding integers) and u8 rows on
    the device 1 byte off every alignment; every result also equals the f32 search with the L1 chain on the same rows"""
    T = modsx.fginn_l1_geometry(257, 1000)["tile"]
    assert T == 128
    c = FC.integer_case(257, 2 * T + 1, 31)
    records = 0
    for n2 in (1, 3, 4, T - 1, T, T + 1, 2 * T + 1):
        tiles = (n2 + T - 1) // T
        dq, dt = _dev(c["q"], np.uint8, 1), _dev(c["t"][:n2], np.uint8, 1)
        assert dq[1] % 2 == 1 and dt[1] % 2 == 1
        for nn in (2, 4, 50):
            ref = LM.match_int(c, nn, n2=n2)
            records += len(ref)
            FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"][:n2], c["pos"][:n2], c["ratio"], c["cd"], nn, dist=modsx.DIST_L1), ref)
            for n1 in N1S:
                want = ref[ref["q"] < n1]
                for splits in (1, 2, 3, 0):
                    r = _u8(ctx, c, nn, splits, n1, n2)
                    g = r["geometry"]
                    assert g == modsx.fginn_l1_geometry(n1, n2, splits) and g["tile"] == T and g["tiles"] == tiles
                    FC.same_tents(r["tentatives"], want)
                FC.same_tents(ctx.match_fginn_l1_device(dq[1], n1, dt[1], n2, c["pos"][:n2], c["ratio"], c["cd"], nn), want)
                FC.same_tents(ctx.match_fginn_l1(c["q"][:n1], c["t"][:n2], c["pos"][:n2], c["ratio"], c["cd"], nn), want)
        idx, dist = LM.knn_l1_int(c["q"], c["t"][:n2], 4)
        assert np.array_equal(_u8(ctx, c, 50, 0, None, n2)["top4"], _keys(idx, dist))
    assert records > 100


@pytest.mark.parametrize("nn", [2, 4, 50])
def test_u8_walk_cases_take_the_stage_they_claim(modsx, ctx, nn):
    c = LC.walk_case(integer=True)
    ref = LM.match_int(c, nn)
    ia, da = LM.knn_l1_int(c["q"], c["t"], len(c["t"]))
    stage = FC.expected_stage(ia, da, c["pos"], c["ratio"], c["cd"], nn)
    tiles = modsx.fginn_l1_geometry(len(c["q"]), len(c["t"]))["tiles"]
    assert tiles >= 2
    for splits in (0, 1, 2, 3):
        r = _u8(ctx, c, nn, splits)
        FC.same_tents(r["tentatives"], ref)
        assert np.array_equal(r["stage"], stage), splits
        for q, name in c["expect"].items():
            assert r["stage"][q] == (LC.EXPECT_STAGE_NN50[name] if nn == 50 else 0), name
        assert r["resolve"] == int((stage >= 1).sum()) and r["by_count"] == int((stage == 2).sum()) and r["records"] == len(ref)
        assert np.array_equal(r["top4"], _keys(ia[:, :4], da[:, :4]))
        f = _f32(ctx, modsx, c, nn, splits)
        FC.same_tents(f["tentatives"], r["tentatives"])
        assert np.array_equal(f["top4"], r["top4"]) and np.array_equal(f["stage"], r["stage"])
    if nn == 50:
        r = _u8(ctx, c, nn, 0, stage_mask=1)
        FC.same_tents(r["tentatives"], ref[stage[ref["q"]] == 0])
        assert len(r["tentatives"]) < len(ref)


@pytest.mark.parametrize("splits", [0, 1, 2, 3, 1 << 20])
def test_u8_planted_ties_across_tile_and_split_edges(modsx, ctx, splits):
    n1 = 70
    T = modsx.fginn_l1_geometry(n1, 1000)["tile"]
    geo = modsx.fginn_l1_geometry(n1, LC.TIE_TILES * T - 2, splits)
    c = LC.tie_case(geo, n1, 128, integer=True)
    r = _u8(ctx, c, 50, splits)
    assert r["geometry"] == geo
    FC.same_tents(r["tentatives"], LM.match_int(c, 50))
    for qi, (a, b) in enumerate(c["pairs"]):
        k = r["top4"][qi]
        assert (int(k[0]) & 0xffffffff, int(k[1]) & 0xffffffff) == (a, b) and k[0] >> np.uint64(32) == k[1] >> np.uint64(32)
    FC.same_tents(_f32(ctx, modsx, c, 50, 0)["tentatives"], r["tentatives"])


def test_u8_saturating_rows(modsx, ctx):
    """rows of all 255 against rows of all 0: 255 in every column, the sum 32640"""
    c = LC.saturating_case()
    ref = LM.match_int(c, 50)
    assert len(ref) > 20
    for splits in (0, 1, 2):
        r = _u8(ctx, c, 50, splits)
        FC.same_tents(r["tentatives"], ref)
    idx, dist = LM.knn_l1_int(c["q"], c["t"], 4)
    assert np.array_equal(r["top4"], _keys(idx, dist))
    FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], 50, dist=modsx.DIST_L1), ref)
    # nothing but the extremes: query all 255 against trains all 0 (and the other way round)
    q = np.full((3, 128), 255, np.float32)
    q[1] = 0
    t = np.zeros((5, 128), np.float32)
    t[4] = 255
    pos = np.zeros((5, 2))
    r = ctx.debug_match_fginn_l1(q, t, pos, 0.8, 30.0, 50)
    big = np.uint64(np.float32(32640).view(np.uint32)) << np.uint64(32)
    assert list(r["top4"][0]) == [np.uint64(4), big | np.uint64(0), big | np.uint64(1), big | np.uint64(2)]
    assert list(r["top4"][1]) == [np.uint64(0), np.uint64(1), np.uint64(2), np.uint64(3)]
    rec = r["tentatives"][r["tentatives"]["q"] == 0][0]
    assert rec["d1"] == 0 and rec["d2"] == 32640.0 and rec["tj"] == 0
    du = _dev(np.r_[q, t], np.uint8, 3)
    FC.same_tents(ctx.match_fginn_l1_device(du[1], 3, du[1] + 3 * 128, 5, pos), r["tentatives"])


def test_u8_refusals_leave_the_context_usable(modsx, ctx):
    c = FC.integer_case(65, 130, 3)
    q, t, pos = c["q"], c["t"], c["pos"]
    ok = LM.match_int(c, 50)
    dq, dt = _dev(q, np.uint8, 0), _dev(t, np.uint8, 0)
    again = lambda: FC.same_tents(ctx.match_fginn_l1(q, t, pos), ok)
    for bad in (np.nan, np.inf, 0.5, -1.0, 256.0, 254.5):      # what modsx_match_fginn refuses
        for side in (0, 1):
            rows = [q.copy(), t.copy()]
            rows[side][5, 7] = bad
            _refused(ctx, lambda: ctx.match_fginn_l1(rows[0], rows[1], pos), again)
            _refused(ctx, lambda: ctx.debug_match_fginn_l1(rows[0], rows[1], pos), again)
            with pytest.raises(RuntimeError, match=r"\(-1\): .+"):
                ctx.match_fginn(rows[0], rows[1], pos)
    for nn in (1, 257, 0, -3):
        _refused(ctx, lambda: ctx.match_fginn_l1(q, t, pos, nn=nn), again)
        _refused(ctx, lambda: ctx.match_fginn_l1_device(dq[1], len(q), dt[1], len(t), pos, nn=nn), again)
    for ratio in (float("nan"), 1.0, 1.5, -1.0, float("inf")):      # the "all points" branch stays refused under L1
        _refused(ctx, lambda: ctx.match_fginn_l1(q, t, pos, ratio=ratio), again)
        _refused(ctx, lambda: ctx.match_fginn_l1_device(dq[1], len(q), dt[1], len(t), pos, ratio=ratio), again)
    regs = np.zeros(len(q), modsx.REGION)
    _refused(ctx, lambda: ctx.match_regions_l1(regs, q, regs, q, modsx.default_pair_params(match_ratio=1.0)), again)
    _refused(ctx, lambda: ctx.match_regions_l1(regs, q + 0.5, regs, q, modsx.default_pair_params()), again)
    _refused(ctx, lambda: ctx.debug_match_fginn_l1(q, t, pos, stage_mask=2), again)
    e, ep = np.zeros((0, 128), np.float32), np.zeros((0, 2))
    assert len(ctx.match_fginn_l1(e, t, pos)) == 0 and len(ctx.match_fginn_l1(q, e, ep)) == 0
    assert len(ctx.match_fginn_l1_device(0, 0, dt[1], len(t), pos)) == 0 and len(ctx.match_fginn_l1_device(dq[1], len(q), 0, 0, ep)) == 0
    assert len(ctx.match_fginn_f32(e[:, :36], t[:, :36], pos, dist=modsx.DIST_L1)) == 0


# ---- production geometry ---------------------------------------------------------------------------------------------------
def _sample(n1, rs):
    """256 queries: the first and last query of the first and last workgroup, and a seeded draw of the others"""
    first, last = (n1 - 1) // 256 * 256, n1 - 1
    must = sorted({0, 255, first, last})
    rest = np.setdiff1d(np.arange(n1), must)
    return np.sort(np.r_[must, rs.choice(rest, 256 - len(must), replace=False)]).astype(np.int64)


def _sampled(c, sel, knn):
    """the model's records of the queries sel, with their own indices"""
    idx, dist = knn(c["q"][sel], c["t"])
    rows, _ = FC.walk(idx, dist, c["pos"], c["ratio"], c["cd"], 50)
    ref = LM.tents(rows)
    ref["q"] = sel[ref["q"]]
    return ref


def _knn_l1_int_big(q, t, nn):
    """LM.knn_l1_int for a sample too large for its loop: integer sums in f64 are exact in any order (torch.cdist on the CPU);
    the first rows are held to LM.knn_l1_int itself"""
    import torch
    d = torch.cdist(torch.from_numpy(q.astype(np.float64)), torch.from_numpy(t.astype(np.float64)), p=1).numpy()
    assert d.max() < 1 << 24 and np.array_equal(d, np.round(d))
    idx, dist = FC._sorted_knn(d.astype(np.float32), nn)
    i8, d8 = LM.knn_l1_int(q[:8], t, nn)
    assert np.array_equal(idx[:8], i8) and np.array_equal(dist[:8], d8)
    return idx, dist


def test_production_geometry_f32_l1(modsx, ctx):
    """the smallest n2 at n1 = 2049 (nine workgroups along the queries) with at least 2 splits of at least 2 tiles.  The model of
    all 2049 x 7297 pairs takes too long for a test: a sample of 256 queries is held to it."""
    n1, n2, dim = 2049, 7297, 128
    g = modsx.fginn32_geometry(n1, n2, dim)
    assert g["splits"] >= 2 and g["tiles_per_split"] >= 2 and modsx.fginn32_geometry(n1, n2 - 1, dim)["tiles_per_split"] == 1
    c = FC.unit_case(n1, n2, dim, 21)
    r = _f32(ctx, modsx, c)
    assert r["geometry"] == g
    sel = _sample(n1, np.random.RandomState(1))
    ref = _sampled(c, sel, lambda q, t: LM.knn(q, t, 50, "l1"))
    assert len(ref) > 30
    got = r["tentatives"]
    FC.same_tents(got[np.isin(got["q"], sel)], ref)
    assert 2 * len(ref) < len(got) < n1
    dq, dt = _dev(c["q"], np.float32, 4), _dev(c["t"], np.float32, 4)
    FC.same_tents(ctx.match_fginn_f32_device(dq[1], n1, dt[1], n2, dim, c["pos"], c["ratio"], c["cd"], 50, dist=modsx.DIST_L1), got)


def test_production_geometry_u8(modsx, ctx):
    """the same for the byte search (tiles of 128 trains): n2 = 29185.  A sample of 256 queries is held to the integer model, and
    EVERY query to the f32 search with the L1 chain on the same rows."""
    n1, n2 = 2049, 29185
    g = modsx.fginn_l1_geometry(n1, n2)
    assert g["splits"] >= 2 and g["tiles_per_split"] >= 2 and modsx.fginn_l1_geometry(n1, n2 - 1)["tiles_per_split"] == 1
    c = FC.integer_case(n1, n2, 22)
    r = _u8(ctx, c)
    assert r["geometry"] == g
    got = r["tentatives"]
    f = _f32(ctx, modsx, c)
    FC.same_tents(f["tentatives"], got)
    assert np.array_equal(f["top4"], r["top4"])
    sel = _sample(n1, np.random.RandomState(2))
    ref = _sampled(c, sel, lambda q, t: _knn_l1_int_big(q, t, 50))
    assert len(ref) > 30
    FC.same_tents(got[np.isin(got["q"], sel)], ref)
    dq, dt = _dev(c["q"], np.uint8, 1), _dev(c["t"], np.uint8, 1)
    FC.same_tents(ctx.match_fginn_l1_device(dq[1], n1, dt[1], n2, c["pos"], c["ratio"], c["cd"], 50), got)


# ---- the fused call ----------------------------------------------------------------------------------------------------------
def _planted_pair(modsx, integer, n=600, seed=5):
    """n regions per side: 400 of the second side are the first side's under a homography (descriptor + noise), the rest is clutter"""
    rs = np.random.RandomState(seed)
    H = np.array([[1.1, 0.05, 20], [-0.03, 0.95, -10], [1e-5, 2e-5, 1]])
    p1 = rs.uniform(20, 900, (n, 2))
    x = np.c_[p1, np.ones(n)] @ H.T
    p2 = x[:, :2] / x[:, 2:] + rs.normal(0, 0.5, (n, 2))
    if integer:
        d1 = rs.randint(0, 256, (n, 128)).astype(np.float32)
        d2 = np.clip(d1 + rs.randint(-25, 26, (n, 128)), 0, 255).astype(np.float32)
        d2[400:] = rs.randint(0, 256, (n - 400, 128))
    else:
        d1 = rs.randn(n, 144).astype(np.float32)
        d2 = (d1 + 0.25 * rs.randn(n, 144)).astype(np.float32)
        d2[400:] = rs.randn(n - 400, 144)
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


@pytest.mark.parametrize("path", ["f32", "u8"])
def test_fused_call_is_match_plus_duplicate_filter_plus_loransac(modsx, ctx, path):
    r1, d1, r2, d2 = _planted_pair(modsx, path == "u8")
    par = modsx.default_pair_params(ransac_seed=1)
    fused = (lambda a, da, b, db: ctx.match_regions_l1(a, da, b, db, par)) if path == "u8" else \
        (lambda a, da, b, db: ctx.match_regions_f32(a, da, b, db, par, dist=modsx.DIST_L1))
    got = fused(r1, d1, r2, d2)
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    if path == "u8":
        tent = ctx.match_fginn_l1(d1, d2, pos2, par.match_ratio, par.contradDist, par.nn)
    else:
        tent = ctx.match_fginn_f32(d1, d2, pos2, par.match_ratio, par.contradDist, par.nn, dist=modsx.DIST_L1)
    FC.same_tents(tent, LM.match(dict(q=d1, t=d2, pos=pos2, ratio=par.match_ratio, cd=par.contradDist), par.nn, "l1"))
    assert len(tent) >= 300
    pts = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                    r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = modsx.duplicate_filtering(pts, tent["ratio"], par.duplicateDist, True)
    sel = order[keep]
    tu, pu = tent[sel], pts[sel]
    rr = modsx.loransac_h(pu, laf_of(r1, tu["q"]), laf_of(r2, tu["t0"]), err_threshold=par.err_threshold, confidence=par.confidence,
                          max_samples=par.max_samples, lo=par.localOptimization, hlaf_coef=par.HLAFCoef, sym_check=par.doSymmCheck, seed=1,
                          error_type=par.errorType)
    assert got["n_regions"] == (len(r1), len(r2)) and got["n_tentatives"] == len(tent) and got["n_unique"] == len(tu)
    FC.same_tents(got["tentatives"], tu)
    assert np.array_equal(got["ransac_inlier"], rr["inl"]) and np.array_equal(got["verified"], rr["keep"])
    assert got["n_verified"] == rr["n"] and got["n_ransac_inliers"] == int(rr["inl"].sum()) and got["ransac_samples"] == rr["samples"]
    assert np.array_equal(got["H"], rr["H"]) and got["n_verified"] >= 200
    for a, b in ((0, len(r1)), (len(r1), 0)):                      # an empty side
        r = fused(r1[:a], d1[:a], r2[:b], d2[:b])
        assert r["n_regions"] == (a, b) and r["n_tentatives"] == 0 and r["n_unique"] == 0 and r["n_verified"] == 0
        assert (r["H"] == -1).all() and len(r["tentatives"]) == 0
