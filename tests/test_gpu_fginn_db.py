"""GPU: FGINN matching against a descriptor database (MatchFlannFGINNPlusDB, matching.cpp:462-572; kernels_dbnn.hip).

The reference is tests/fginn_db_model.py (pinned to the oracle on the CPU by tests/test_fginn_db_model_cpu.py).  Every
comparison is field-wise and exact; d2byDB is exact."""
import numpy as np
import pytest

from common import laf_of, need_ref, normH, oracle_features, same_records, DESC_NAME_ORDER, DET_NAME_ORDER
import fginn_db_model as M

pytestmark = pytest.mark.gpu


def _u8(a):
    return np.ascontiguousarray(a, np.float32).astype(np.uint8)


# ---- 1. stand-alone matcher on real descriptors ----------------------------------------------------------------------------------
def test_match_fginn_db_bit_exact_on_real_descriptors(ctx, oracle, small_pair):
    P = M.planted_input(oracle, small_pair)
    d1, d2, pos2 = P["d1"], P["d2"], P["pos2"]
    db = ctx.db_create(_u8(P["db"]))
    assert db.rows == len(P["db"])
    ddb = M.db_nearest(d1, P["db"])
    assert np.array_equal(ctx.db_nearest(db, d1), ddb)
    for ratio, cd in ((0.8, 30.0), (0.9, 30.0), (0.6, 3.0), (1.0, 30.0)):
        ref, rd = M.match_fginn_db(d1, d2, pos2, None, ratio, cd, ddb=ddb)
        got, gd = ctx.match_fginn_db(d1, d2, pos2, db, ratio, cd)
        assert len(ref) > 5
        M.same_tents(got, ref)
        assert np.array_equal(gd, rd)
    # the database decides something (ratio 0.8): it rejects, it keeps, it raises ratios; the planted cases fall as stated
    plain = ctx.match_fginn(d1, d2, pos2, 0.8, 30.0)
    got, _ = ctx.match_fginn_db(d1, d2, pos2, db, 0.8, 30.0)
    kept = np.isin(plain["q"], got["q"])
    print("plain %d kept %d raised %d" % (len(plain), len(got), (got["ratio"] > plain["ratio"][kept]).sum()))
    assert (~kept).sum() * 5 >= len(plain) and kept.sum() * 5 >= len(plain)
    assert (got["ratio"] > plain["ratio"][kept]).sum() * 5 >= len(got)
    assert P["q_nan"] in got["q"]
    assert P["q_inf"] in plain["q"] and P["q_inf"] not in got["q"]
    # the same on descriptors that already live in HBM
    import torch
    t1, t2 = torch.from_numpy(_u8(d1)).cuda(), torch.from_numpy(_u8(d2)).cuda()
    dev, dd = ctx.match_fginn_db_device(t1.data_ptr(), len(d1), t2.data_ptr(), len(d2), pos2, db, 0.8, 30.0)
    M.same_tents(dev, got)
    assert np.array_equal(dd, ddb[got["q"]].astype(np.float64))
    db.free()
    assert db.rows == 0


# ---- 2. ties and edges -------------------------------------------------------------------------------------------------------------
def _row_at_distance(q, D):
    """a descriptor (integers 0..255) at squared distance exactly D from q"""
    row = q.astype(np.int64).copy()
    for i in range(128):
        if D == 0:
            break
        room = max(int(row[i]), 255 - int(row[i]))
        k = min(int(np.sqrt(D)), room)
        while k * k > D:
            k -= 1
        row[i] += k if row[i] + k <= 255 else -k
        D -= k * k
    assert D == 0
    return row.astype(np.float32)


def test_match_fginn_db_ties_edges_and_exact_thresholds(ctx, oracle, small_pair):
    rs = np.random.RandomState(9)
    for (n1, n2), m in zip(((1, 50), (33, 95), (70, 257), (5, 64), (40, 130)), (1, 31, 32, 33, 257)):
        # low-entropy descriptors: many exact distance ties, duplicates, zero distances -- also against the database
        d1 = rs.randint(0, 3, (n1, 128)).astype(np.float32) * 40
        d2 = rs.randint(0, 3, (n2, 128)).astype(np.float32) * 40
        d2[n2 // 2:] = d2[: n2 - n2 // 2]
        d1[0] = d2[3]
        dbr = rs.randint(0, 3, (m, 128)).astype(np.float32) * 40
        if m > 1:
            dbr[m - 1] = d1[0]                                  # exact hit in the last row (the NaN case on a tie-heavy input)
        pos2 = rs.uniform(0, 60, (n2, 2))
        db = ctx.db_create(dbr)                                 # the f32 form
        assert np.array_equal(ctx.db_nearest(db, d1), M.db_nearest(d1, dbr))
        for ratio, cd in ((0.8, 30.0), (0.95, 80.0), (0.8, 5.0), (1.0, 30.0)):
            ref, rd = M.match_fginn_db(d1, d2, pos2, dbr, ratio, cd)
            got, gd = ctx.match_fginn_db(d1, d2, pos2, db, ratio, cd)
            M.same_tents(got, ref)
            assert np.array_equal(gd, rd)
        db.free()
    # dDB == d0, dDB at the exact integer threshold of the ratio test, and one below it: one-row databases on real descriptors
    a, b, _ = small_pair
    _, _, d1 = oracle_features(oracle, a)
    _, r2, d2 = oracle_features(oracle, b)
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    ratio, sq = 0.8, 0.8 * 0.8
    plain = ctx.match_fginn(d1, d2, pos2, ratio, 30.0)
    t = plain[plain["d1"] > 1000][0]
    q, d0 = int(t["q"]), int(t["d1"])
    Dt = int(d0 / sq) - 3
    while not np.float64(np.float32(d0) / np.float32(Dt)) <= sq:      # smallest integer distance that passes
        Dt += 1
    assert np.float64(np.float32(d0) / np.float32(Dt - 1)) > sq
    for D, keeps in ((d0, False), (Dt - 1, False), (Dt, True)):
        dbr = _row_at_distance(d1[q], D)[None]
        assert M.db_nearest(d1[q][None], dbr)[0] == D
        db = ctx.db_create(_u8(dbr))
        ref, rd = M.match_fginn_db(d1, d2, pos2, dbr, ratio, 30.0)
        got, gd = ctx.match_fginn_db(d1, d2, pos2, db, ratio, 30.0)
        M.same_tents(got, ref)
        assert np.array_equal(gd, rd)
        assert (q in got["q"]) == keeps
        if keeps:
            assert gd[list(got["q"]).index(q)] == D
        db.free()
    # n1 = 0
    db = ctx.db_create(_u8(d2[:7]))
    got, gd = ctx.match_fginn_db(np.zeros((0, 128)), d2, pos2, db)
    assert len(got) == 0 and len(gd) == 0
    assert len(ctx.db_nearest(db, np.zeros((0, 128)))) == 0
    db.free()


# ---- 3. the 1-NN kernel at size ---------------------------------------------------------------------------------------------------------
def _sift_like(rs, protos, n):
    """sparse prototypes plus jitter, u8"""
    out = np.empty((n, 128), np.uint8)
    for s in range(0, n, 1 << 16):
        c = min(1 << 16, n - s)
        p = protos[rs.randint(0, len(protos), c)].astype(np.int16)
        out[s:s + c] = np.clip(p + rs.randint(-6, 7, (c, 128), dtype=np.int16), 0, 255)
    return out


def _packed_slot_rows(dbr):
    """slot -> row of the packed database (kernels_dbnn.hip: rows of even sum first, then odd, each class in row order and padded
    to whole stages of 4 tiles of 32 rows), and the tile count"""
    par = dbr.sum(1, dtype=np.int64) & 1
    ev, od = np.flatnonzero(par == 0), np.flatnonzero(par == 1)
    TE = ((len(ev) + 31) // 32 + 3) // 4 * 4
    TO = ((len(od) + 31) // 32 + 3) // 4 * 4
    slot = -np.ones((TE + TO) * 32, np.int64)
    slot[:len(ev)] = ev
    slot[TE * 32:TE * 32 + len(od)] = od
    return slot, TE + TO, par


def test_db_nearest_at_size(ctx):
    rs = np.random.RandomState(2024)
    protos = (rs.randint(0, 256, (4096, 128)) * (rs.rand(4096, 128) < 0.35)).astype(np.uint8)
    n, nq = (1 << 20) + 37, 2085
    dbr = _sift_like(rs, protos, n)
    qs = np.clip(protos[rs.randint(0, 4096, nq)].astype(np.int16) + rs.randint(-40, 41, (nq, 128)), 0, 255).astype(np.uint8)
    # planted minima: first row, last row, both sides of a 32-row tile border and of a split border of k_dbnn_min's geometry (nq
    # selected queries: 9 blocks of 256, 512 workgroups -> 56 splits of whole 4-tile stages), and one exact hit.  A planted row
    # keeps the parity of the row it replaces, so that the packed layout does not move.
    slot, ntiles, par = _packed_slot_rows(dbr)
    S = min(512 // ((nq + 255) // 256), ntiles // 12)
    tps = ((ntiles + S - 1) // S + 3) // 4 * 4
    assert S > 8 and tps * 32 < len(slot)
    spots = [0, n - 1, int(slot[32 * 5 - 1]), int(slot[32 * 5]), int(slot[tps * 32 - 1]), int(slot[tps * 32])]
    assert min(spots) >= 0
    for k, row in enumerate(spots):
        v = qs[k].astype(np.int64)
        i = int(np.flatnonzero((v > 0) & (v < 255))[0])
        v[i] += 1
        if (v.sum() & 1) != par[row]:
            j = int(np.flatnonzero((v > 0) & (v < 255))[1])
            v[j] += 1
        dbr[row] = v
    hit = int(np.flatnonzero(par == (qs[10].sum(dtype=np.int64) & 1))[12345])
    dbr[hit] = qs[10]
    assert np.array_equal(_packed_slot_rows(dbr)[0], slot)
    qf = qs.astype(np.float32)
    ref = np.full(nq, np.inf, np.float32)
    arg = np.zeros(nq, np.int64)
    for s in range(0, n, 1 << 15):
        d = M.sqdist_f32(qf, dbr[s:s + (1 << 15)].astype(np.float32))
        m, a = d.min(1), d.argmin(1) + s
        arg = np.where(m < ref, a, arg)
        ref = np.minimum(ref, m)
    for k, row in enumerate(spots):
        assert arg[k] == row and ref[k] in (1, 2), (k, row, arg[k], ref[k])
    assert ref[10] == 0
    assert len(np.unique(ref)) > 500                 # the minima spread widely
    db = ctx.db_create(dbr)
    assert db.rows == n
    got = ctx.db_nearest(db, qf)
    db.free()
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    # the f32 form of the database at 2^16 rows gives the same answers as its u8 form
    sub = dbr[:1 << 16]
    db8, db32 = ctx.db_create(sub), ctx.db_create(sub.astype(np.float32))
    g8, g32 = ctx.db_nearest(db8, qf), ctx.db_nearest(db32, qf)
    db8.free(); db32.free()
    assert np.array_equal(g8, M.db_nearest(qf, sub.astype(np.float32))) and np.array_equal(g32, g8)


# ---- 4. fused paths ------------------------------------------------------------------------------------------------------------------------
def _verify(oracle, r1, r2, tent, seed, dup=2.0):
    pts = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                    r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = oracle.duplicate_filtering(pts, tent["ratio"], dup, True)
    sel = order[keep]
    tu, pu = tent[sel], pts[sel]
    return tu, oracle.loransac_h(pu, laf_of(r1, tu["q"]), laf_of(r2, tu["t0"]), seed=seed)


def _ladder_ref(oracle, a, b, steps, seed, dbr):
    """tests/common.py oracle_ladder with every step run, and the RootSIFT classes (type 1), and no other, matched against the
    database (correspondencebank.cpp:333-341): model records -> duplicate_filtering -> loransac_h"""
    cls, out = {}, None
    for views, ratio, det, descs in steps:
        descs = descs or [(1, ratio)]
        types = [t for t, _ in descs]
        for side, img in enumerate((a, b)):
            r, ds = oracle.detect_describe_views(img, views, params=None, ori=(1.0, 41, 1, 0.8), mser=None, threads=1, descs=types)
            for t, d in zip(types, ds):
                k = cls.setdefault((t, det), dict(acc=[[None, None], [None, None]], tent=None))
                if k["acc"][side][0] is None:
                    k["acc"][side] = [r.copy(), d]
                else:
                    rr = r.copy()
                    rr["id"] += len(k["acc"][side][0]); rr["parent_id"] += len(k["acc"][side][0])
                    k["acc"][side] = [np.concatenate([k["acc"][side][0], rr]), np.concatenate([k["acc"][side][1], d])]
        for t, thr in descs:
            k = cls[(t, det)]
            (r1, d1), (r2, d2) = k["acc"]
            pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
            if t == 1 and dbr is not None:
                k["tent"] = M.match_fginn_db(d1, d2, pos2, dbr, thr, 30.0)[0]
            else:
                k["tent"] = oracle.match_fginn(d1, d2, pos2, thr, 30.0)
        R1, R2, T = [], [], []
        o1 = o2 = 0
        for t in DESC_NAME_ORDER:
            for dkey in DET_NAME_ORDER:
                kk = cls.get((t, dkey))
                if kk is None:
                    continue
                tt = kk["tent"].copy()
                tt["q"] += o1
                for f in ("t0", "t1", "tj"):
                    tt[f] = np.where(tt[f] >= 0, tt[f] + o2, tt[f])
                T.append(tt); R1.append(kk["acc"][0][0]); R2.append(kk["acc"][1][0])
                o1 += len(kk["acc"][0][0]); o2 += len(kk["acc"][1][0])
        r1, r2, tent = np.concatenate(R1), np.concatenate(R2), np.concatenate(T)
        tu, rr = _verify(oracle, r1, r2, tent, seed)
        out = dict(n_regions=(len(r1), len(r2)), n_tentatives=len(tent), tent=tu, rr=rr,
                   per_class={k: len(v["tent"]) for k, v in cls.items()})
    return out


def _same_as_ref(got, ref):
    assert got["n_regions"] == ref["n_regions"] and got["n_tentatives"] == ref["n_tentatives"]
    assert got["n_unique"] == len(ref["tent"])
    for f in ref["tent"].dtype.names:
        assert np.array_equal(got["tentatives"][f], ref["tent"][f]), f
    rr = ref["rr"]
    assert np.array_equal(got["ransac_inlier"], rr["inl"]) and np.array_equal(got["verified"], rr["keep"])
    assert got["n_verified"] == rr["n"]
    assert np.abs(normH(got["H"]) - normH(rr["H"])).max() < 1e-4


def _same_pair_result(got, ref):
    for k in ("n_regions", "n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples"):
        assert got[k] == ref[k], k
    assert same_records(got["tentatives"], ref["tentatives"])
    assert np.array_equal(got["H"], ref["H"]) and np.array_equal(got["verified"], ref["verified"])


def test_fused_paths_with_a_database_attached(ctx, modsx, oracle, small_pair):
    a, b, _ = small_pair
    need_ref(oracle)
    P = M.planted_input(oracle, small_pair)
    dbr = P["db"]
    db = ctx.db_create(_u8(dbr))
    ia, ib = ctx.upload(a), ctx.upload(b)
    seed = 6
    par = modsx.default_pair_params(ransac_seed=seed)
    vo = oracle.set_vs_pars([1.0], [1, 2], 360.0, 0.2, 1, [])
    vm = modsx.set_vs_pars([1.0], [1, 2], 360.0, 0.2, 1, [])
    prev_o, prev_m, steps_o, steps_m = [], [], [], []
    for tilts, descs in (([1], [(1, 0.8), (3, 0.8)]), ([1, 2], [(1, 0.85), (3, 0.8)])):
        so = oracle.set_vs_pars([1.0], tilts, 360.0, 0.2, 1, prev_o)
        sm = modsx.set_vs_pars([1.0], tilts, 360.0, 0.2, 1, prev_m)
        steps_o.append((so, 0.0, 0, descs)); steps_m.append((sm, 0.0, 0, descs))
    plain_pair = ctx.match_pair(ia, ib, par)
    plain_views = ctx.match_pair_views(ia, ib, vm, par)
    plain_ladder, _ = ctx.match_ladder(ia, ib, steps_m, par, min_matches=10 ** 6)
    ctx.set_fginn_db(db)
    try:
        # match_pair: the identity-view pair path
        got = ctx.match_pair(ia, ib, par)
        _, r1, d1 = oracle_features(oracle, a)
        _, r2, d2 = oracle_features(oracle, b)
        pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
        tent = M.match_fginn_db(d1, d2, pos2, dbr, 0.8, 30.0)[0]
        tu, rr = _verify(oracle, r1, r2, tent, seed)
        _same_as_ref(got, dict(n_regions=(len(d1), len(d2)), n_tentatives=len(tent), tent=tu, rr=rr))
        assert got["n_tentatives"] < plain_pair["n_tentatives"]
        # match_pair_views: a short view list (one RootSIFT class)
        got = ctx.match_pair_views(ia, ib, vm, par)
        ref = _ladder_ref(oracle, a, b, [(vo, 0.8, 0, None)], seed, dbr)
        _same_as_ref(got, ref)
        assert got["n_tentatives"] < plain_views["n_tentatives"]
        # match_ladder: two steps that carry RootSIFT + HalfRootSIFT -- the database applies to the RootSIFT class alone, at every
        # re-match: the HalfRootSIFT class has as many records as without a database, the RootSIFT class has fewer
        got, done = ctx.match_ladder(ia, ib, steps_m, par, min_matches=10 ** 6)
        ref = _ladder_ref(oracle, a, b, steps_o, seed, dbr)
        ref_plain = _ladder_ref(oracle, a, b, steps_o, seed, None)
        assert done == 2
        _same_as_ref(got, ref)
        _same_as_ref(plain_ladder, ref_plain)
        assert ref["per_class"][(3, 0)] == ref_plain["per_class"][(3, 0)] > 10
        assert ref["per_class"][(1, 0)] < ref_plain["per_class"][(1, 0)]
        assert got["n_tentatives"] == ref["per_class"][(3, 0)] + ref["per_class"][(1, 0)]
    finally:
        ctx.set_fginn_db(None)
    # detached: the plain path again
    _same_pair_result(ctx.match_pair(ia, ib, par), plain_pair)
    _same_pair_result(ctx.match_pair_views(ia, ib, vm, par), plain_views)
    _same_pair_result(ctx.match_ladder(ia, ib, steps_m, par, min_matches=10 ** 6)[0], plain_ladder)
    # freeing a database that is still attached to the freeing context detaches it
    ctx.set_fginn_db(db)
    db.free()
    _same_pair_result(ctx.match_pair(ia, ib, par), plain_pair)
    ia.free(); ib.free()


# ---- 5. batch equality ---------------------------------------------------------------------------------------------------------------------
def test_match_pairs_views_with_a_database_equals_single_calls(modsx, oracle, small_pair):
    a, b, _ = small_pair
    P = M.planted_input(oracle, small_pair)
    ctxs = [modsx.Context(0) for _ in range(4)]
    db = ctxs[0].db_create(_u8(P["db"]))                # usable by every context of its device
    views = modsx.set_vs_pars([1.0], [1, 2, 3], 360.0, 0.2, 1, [])
    par = modsx.default_pair_params(ransac_seed=9)
    ims = [(ctxs[0].upload(a), ctxs[0].upload(b)), (ctxs[0].upload(b), ctxs[0].upload(a))]
    i1 = [ims[i % 2][0] for i in range(7)]
    i2 = [ims[i % 2][1] for i in range(7)]
    plain = ctxs[0].match_pair_views(i1[0], i2[0], views, par)
    for c in ctxs:
        c.set_fginn_db(db)
    got = modsx.match_pairs_views(ctxs, i1, i2, views, par)
    for i in range(7):
        _same_pair_result(got[i], ctxs[0].match_pair_views(i1[i], i2[i], views, par))
    assert got[0]["n_tentatives"] < plain["n_tentatives"]
    # identity-view batch form
    gp = modsx.match_pairs(ctxs, i1, i2, par)
    for i in range(7):
        _same_pair_result(gp[i], ctxs[0].match_pair(i1[i], i2[i], par))
    # contexts that disagree about the database: an error before any work
    ctxs[2].set_fginn_db(None)
    with pytest.raises(RuntimeError):
        modsx.match_pairs_views(ctxs, i1, i2, views, par)
    with pytest.raises(RuntimeError):
        modsx.match_pairs(ctxs, i1, i2, par)
    for c in ctxs:
        c.set_fginn_db(None)
    _same_pair_result(modsx.match_pairs_views(ctxs, i1[:1], i2[:1], views, par)[0], plain)
    db.free()
    for x, y in ims:
        x.free(); y.free()
    for c in ctxs:
        c.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_database_refusals(ctx, modsx, small_pair):
    rs = np.random.RandomState(1)
    d = rs.randint(0, 255, (40, 128)).astype(np.float32)
    p2 = rs.uniform(0, 60, (40, 2))
    for bad in (d + 0.5, d - 300.0, d + 200.0, np.where(np.arange(128) == 3, np.nan, d)):
        with pytest.raises(RuntimeError):
            ctx.db_create(bad.astype(np.float32))
    with pytest.raises(RuntimeError):
        ctx.db_create(np.zeros((0, 128), np.uint8))
    db = ctx.db_create(d)
    for bad in (d + 0.5, d - 300.0, np.where(np.arange(128) == 3, np.nan, d)):
        with pytest.raises(RuntimeError):
            ctx.match_fginn_db(bad.astype(np.float32), d, p2, db)
        with pytest.raises(RuntimeError):
            ctx.db_nearest(db, bad.astype(np.float32))
    with pytest.raises(RuntimeError):
        ctx.match_fginn_db(d, d, p2, None)
    with pytest.raises(RuntimeError):
        ctx.match_fginn_db(d, d, p2, db, nn=300)
    import torch
    if torch.cuda.device_count() > 1:                   # a database of another device
        other = modsx.Context(1)
        with pytest.raises(RuntimeError):
            other.match_fginn_db(d, d, p2, db)
        with pytest.raises(RuntimeError):
            other.set_fginn_db(db)
        other.close()
    # a sharded call on a context with a database attached: refused at entry on every rank, before any collective
    from mods_amd import distributed as D
    a, b, _ = small_pair
    views = modsx.set_vs_pars([1.0], [1, 2], 360.0, 0.2, 1, [])
    par = modsx.default_pair_params(ransac_seed=4)
    ia, ib = ctx.upload(a), ctx.upload(b)

    def rank_body(r, comm):
        c = comm.ctxs[0]
        c.set_fginn_db(db)
        errs = 0
        for call in (lambda: c.match_pair_views_sharded(comm.comm, ia, ib, views, par, -1),
                     lambda: comm.detect_describe_views_sharded(0, ia, views, par),
                     lambda: c.match_ladder(ia, ib, [(views, 0.8)], par, comm=comm.comm)):
            try:
                call()
            except RuntimeError as e:
                errs += "descriptor database" in str(e)
        c.set_fginn_db(None)
        ok = c.match_pair_views_sharded(comm.comm, ia, ib, views, par, -1)      # detached: the sharded call works again
        return errs, ok["n_tentatives"]

    out = D.run_loopback(2, rank_body)
    ref = ctx.match_pair_views(ia, ib, views, par)
    assert [e for e, _ in out] == [3, 3] and [n for _, n in out] == [ref["n_tentatives"]] * 2
    ia.free(); ib.free()
    db.free()
