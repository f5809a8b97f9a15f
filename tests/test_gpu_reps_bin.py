"""GPU: the binary descriptor classes of stored representations (engine_reps_bin.hip) and the grouped Hamming search
(kernels_hamming.hip k_hamg_*).  Expected records come from tests/hamming_model.py (pinned to the oracle's knn_linear by
tests/test_hamming_model_cpu.py) and from the single-problem entries (Context.match_hamming_device, match_regions_hamming), never
from the code under test.  A representation on another device cannot be made with one GPU; that refusal is not exercised here.

Fault latch: a HIP error met by any test of this module sets _FAULT; every later test then fails at once, before it touches the
GPU -- nothing is retried."""
import numpy as np
import pytest

import hamming_model as HM
import reps_bin_cases as BC
from common import laf_of, normH, same_records

pytestmark = pytest.mark.gpu

HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "hipmemcpy", "hipstream",
                   "hipgetlasterror", "unspecified launch failure", "queue error")
_FAULT = None
HES, MSER, ORBDET, SURFDET = BC.HES, BC.MSER, BC.ORBDET, BC.SURFDET
BRISK, FREAK, ORB = BC.BRISK, BC.FREAK, BC.ORB
ALL = 512.0          # above every distance of 64 bytes: every query gives a record, which exposes first, second, d1 and d2


class _Gpu(object):
    """the body of a test: a device error inside it ends the module's GPU work"""

    def __enter__(self):
        if _FAULT is not None:
            pytest.fail("an earlier test of this module met a device error; nothing more is started on the GPU:\n%s" % _FAULT, pytrace=False)

    def __exit__(self, et, ev, tb):
        global _FAULT
        if ev is not None and isinstance(ev, RuntimeError) and any(m in str(ev).lower() for m in HIP_ERROR_MARKS):
            _FAULT = str(ev)[-1500:]
        return False


def _dev(rows, offset=0):
    """the rows in a torch buffer on the device, `offset` bytes into it: (keep-alive, device pointer)"""
    import torch
    rows = np.ascontiguousarray(rows, np.uint8)
    buf = torch.zeros(rows.size + 32, dtype=torch.uint8, device="cuda")
    buf[offset:offset + rows.size] = torch.from_numpy(rows.reshape(-1)).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _slot(modsx, ctx, rows, det=ORBDET, typ=ORB, seed=0):
    """a fresh representation whose one binary class holds these rows"""
    rep = modsx.Rep(ctx)
    if len(rows):
        assert rep.append_bin(BC.regs_for(modsx, len(rows), seed), rows, det, typ) == len(rows)
    return rep


def _free(*reps):
    for r in reps:
        r.free()


# ---- 1. the stored match against the model and the single call ---------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [1, 4, 5, 8, 16, 17, 32, 33, 64])
def test_stored_match_equals_the_model_and_the_single_call(modsx, ctx, nbytes):
    with _Gpu():
        T = BC.tile_len(nbytes)
        assert T == modsx.hamming_geometry(4, 8, nbytes)["tile"]
        q, t = HM.random_rows(257, 2 * T + 3, nbytes, 40 + nbytes)
        (kq, pq), (kt, pt) = _dev(q, nbytes % 2), _dev(t, nbytes % 2)
        det, typ = [(ORBDET, ORB), (HES, BRISK), (MSER, FREAK), (SURFDET, ORB)][nbytes % 4]
        rq = {n1: _slot(modsx, ctx, q[:n1], det, typ) for n1 in (1, 2, 255, 256, 257)}
        cut = 0
        for n2 in (2, T - 1, T, T + 1, 2 * T + 3):
            rt = _slot(modsx, ctx, t[:n2], det, typ)
            nn2 = HM.knn2(q, t[:n2])
            low = max(0.5, float(np.median(nn2[:, 1])) - 1)       # a threshold that cuts the list
            for n1, r in rq.items():
                for thr in (ALL, low):
                    ref = HM.tentatives(nn2[:n1], thr)
                    HM.same_tents(ctx.rep_match_hamming(r, rt, det, typ, thr), ref)
                    HM.same_tents(ctx.match_hamming_device(pq, n1, pt, n2, nbytes, thr), ref)
                    cut += thr != ALL and len(ref) < n1
                assert len(HM.tentatives(nn2[:n1], ALL)) == n1
            rt.free()
        assert cut > 5
        _free(*rq.values())


# ---- 2. appends ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [32, 5])
def test_appends_in_three_cuts_across_the_first_capacity(modsx, ctx, nbytes):
    with _Gpu():
        n2 = modsx.REP_BIN_FIRST_ROWS + 2
        q, t = HM.random_rows(70, n2, nbytes, 9 + nbytes)
        regs = BC.regs_for(modsx, n2, 3)
        whole, parts, rq = modsx.Rep(ctx), modsx.Rep(ctx), _slot(modsx, ctx, q)
        assert whole.append_bin(regs, t) == n2
        assert parts.regions_bin()[1].shape == (0, 0) and parts.count_bin() == 0            # an empty class has no width yet
        assert parts.append_bin(regs[:0], t[:0]) == 0 and parts.count_bin() == 0            # n == 0: a no-op
        before = ctx.hamming_group_counters()["rows_packed"]
        at = 0
        for k, n in enumerate((1, 4094, 3)):                      # the third crosses 4096
            if k == 1:
                keep, p = _dev(t[at:at + n], 1)                   # from HBM, one byte off every alignment
                assert p % 2 == 1 and parts.append_bin_device(regs[at:at + n], p, nbytes) == n
            elif k == 2:
                assert parts.append_bin(regs[at:at + n], t[at:at + n].astype(np.float32)) == n      # f32 holding integers
            else:
                assert parts.append_bin(regs[at:at + n], t[at:at + n]) == n
            at += n
            assert parts.count_bin() == at
        assert at == n2 and ctx.hamming_group_counters()["rows_packed"] - before == n2
        ref = HM.match(q, t, ALL)
        for rep in (whole, parts):
            gr, gd = rep.regions_bin()
            assert gd.dtype == np.uint8 and np.array_equal(gd, t) and same_records(gr, regs)
            HM.same_tents(ctx.rep_match_hamming(rq, rep, distance_threshold=ALL), ref)
            HM.same_tents(ctx.rep_match_hamming(rep, rq, distance_threshold=ALL), HM.match(t, q, ALL))      # the same buffer as queries
        keep3, p3 = _dev(t[:7], 3)                                # three bytes off
        dev3 = modsx.Rep(ctx)
        assert dev3.append_bin_device(regs[:7], p3, nbytes) == 7 and np.array_equal(dev3.regions_bin()[1], t[:7])
        _free(whole, parts, rq, dev3)


def _bad_appends(modsx, rep, regs, nbytes):
    """three appends that must fail: f32 rows holding 0.5, a wrong width, dtype 2"""
    half = np.full((4, nbytes), 0.5, np.float32)
    with pytest.raises(RuntimeError, match=r"\(-1\): .+0\.\.255"):
        rep.append_bin(regs[:4], half)
    if rep.count_bin():
        with pytest.raises(RuntimeError, match=r"\(-1\): .+another width"):
            rep.append_bin(regs[:4], np.ones((4, nbytes - 1 if nbytes > 1 else 2), np.uint8))
    with pytest.raises(RuntimeError, match=r"\(-1\): .+nbytes"):
        rep.append_bin(regs[:4], np.ones((4, 65), np.uint8))
    with pytest.raises(RuntimeError, match=r"\(-1\): .+dtype"):
        rep.append_bin(regs[:4], np.ones((4, nbytes), np.uint8), dtype=2)


def test_a_failed_append_changes_neither_the_read_back_nor_a_match(modsx, ctx):
    with _Gpu():
        nbytes = 32
        q, t = HM.random_rows(70, 300, nbytes, 21)
        regs = BC.regs_for(modsx, 300, 4)
        rq, rt = _slot(modsx, ctx, q), modsx.Rep(ctx)
        rt.append_bin(regs, t)
        ref = HM.match(q, t, ALL)
        _bad_appends(modsx, rt, regs, nbytes)
        gr, gd = rt.regions_bin()
        assert rt.count_bin() == 300 and np.array_equal(gd, t) and same_records(gr, regs)
        HM.same_tents(ctx.rep_match_hamming(rq, rt, distance_threshold=ALL), ref)
        # a class that is still empty after failed appends has no width: it takes any width next
        fresh = modsx.Rep(ctx)
        _bad_appends(modsx, fresh, regs, nbytes)
        assert fresh.count_bin() == 0 and fresh.regions_bin()[1].shape == (0, 0)
        assert fresh.append_bin(regs[:9], t[:9, :5]) == 9 and np.array_equal(fresh.regions_bin()[1], t[:9, :5])
        _free(rq, rt, fresh)


# ---- 3. padding is never a neighbour ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [32, 5, 64])
def test_zero_padding_rows_are_never_neighbours(modsx, ctx, nbytes):
    with _Gpu():
        T = BC.tile_len(nbytes)
        zq = _slot(modsx, ctx, np.zeros((258, nbytes), np.uint8))
        built = {}
        # a fresh class; a class grown past the first capacity; a class after failed appends.  n2 is no multiple of the tile
        for name, n2 in (("fresh", T + 1), ("grown", modsx.REP_BIN_FIRST_ROWS + T // 2 + 1), ("failed", 2 * T + 3)):
            t = BC.nonzero_rows(n2, nbytes, 5 + n2 % 97)
            regs = BC.regs_for(modsx, n2, 6)
            rep = modsx.Rep(ctx)
            if name == "grown":
                rep.append_bin(regs[:4000], t[:4000]); rep.append_bin(regs[4000:], t[4000:])
            elif name == "failed":
                _bad_appends(modsx, rep, regs, nbytes)
                rep.append_bin(regs[:T], t[:T])
                _bad_appends(modsx, rep, regs, nbytes)
                rep.append_bin(regs[T:], t[T:])
            else:
                rep.append_bin(regs, t)
            assert n2 % T != 0 and rep.count_bin() == n2
            built[name] = (rep, t, n2)
        got = ctx.rep_match_group_hamming(zq, [built[k][0] for k in ("fresh", "grown", "failed")], distance_threshold=ALL)
        for g, k in zip(got, ("fresh", "grown", "failed")):
            rep, t, n2 = built[k]
            assert len(g) == 258
            for f in ("t0", "tj", "t1"):
                assert (g[f] >= 0).all() and (g[f] < n2).all(), (k, f)
            assert (g["d1"] > 0).all() and (g["d2"] > 0).all(), k
            HM.same_tents(g, HM.match(np.zeros((258, nbytes), np.uint8), t, ALL))
            HM.same_tents(ctx.rep_match_hamming(zq, rep, distance_threshold=ALL), g)
        _free(zq, *[v[0] for v in built.values()])


# ---- 4. groups -----------------------------------------------------------------------------------------------------------------------
def _delta(ctx, before):
    now = ctx.hamming_group_counters()
    return {k: now[k] - before[k] for k in now}


@pytest.mark.parametrize("nbytes", [32, 5])
def test_groups_equal_the_single_partner_tap_in_every_rotation(modsx, ctx, nbytes):
    with _Gpu():
        T = BC.tile_len(nbytes)
        sizes = [2, T + 1, 0, 2 * T + 3]
        q = HM.random_rows(257, 2, nbytes, 77)[0]
        trains = [HM.random_rows(2, n, nbytes, 80 + i)[1] for i, n in enumerate(sizes)]
        rq = _slot(modsx, ctx, q)
        parts = [_slot(modsx, ctx, t, seed=i) for i, t in enumerate(trains)]
        refs = [HM.match(q, t, ALL) for t in trains]
        assert [len(r) for r in refs] == [257, 257, 0, 257]
        for G in (1, 2, 3, 4):
            for rot in range(4):
                order = [(rot + k) % 4 for k in range(G)]
                before = ctx.hamming_group_counters()
                got = ctx.rep_match_group_hamming(rq, [parts[i] for i in order], distance_threshold=ALL)
                live = sum(1 for i in order if sizes[i])
                assert _delta(ctx, before) == dict(launch_sets=1 if live else 0, problems=live, rows_packed=0, match_pack_launches=0), order
                assert len(got) == G
                for g, i in zip(got, order):
                    HM.same_tents(g, refs[i])
                    HM.same_tents(g, ctx.rep_match_hamming(rq, parts[i], distance_threshold=ALL))
        # an empty query class: no launch, no record
        empty = modsx.Rep(ctx)
        before = ctx.hamming_group_counters()
        assert [len(g) for g in ctx.rep_match_group_hamming(empty, parts, distance_threshold=ALL)] == [0, 0, 0, 0]
        assert _delta(ctx, before)["launch_sets"] == 0
        _free(rq, empty, *parts)


def test_large_group_with_planted_ties_at_tile_and_split_edges(modsx, ctx):
    with _Gpu():
        nbytes, n1, big = 32, 8192, 20011
        small = [300, 2, 131]
        geo = modsx.hamming_group_geometry(n1, [big] + small, nbytes)
        T = geo["tile"]
        tiles, S, tps = geo["per_problem"][0]
        assert geo["gx"] == 32 and S > 3 and tps >= 2 and tiles == -(-big // T)      # several splits per partner, several query blocks
        first = [s for s in geo["splits"] if s[0] == 0]
        start = first[1][1] * T                                   # the first row of the big partner's second split
        assert first[0][1:] == (0, tps) and start == tps * T
        # the `copies` query: its nearest train stands on both sides of the first tile edge.  Query 6: on both sides of the split edge
        q, t, info = HM.planted(n1, big, nbytes, [T - 1, T])
        rs = np.random.RandomState(3)
        q[6] = rs.randint(0, 256, nbytes)
        t[start - 1] = t[start] = HM.flip(q[6], [3, 33])
        assert start - 1 not in info["copies"] and all(start - 1 > v for v in (info["tie_second"][2], info["above_max"]))
        trains = [t] + [HM.random_rows(2, n, nbytes, 60 + n)[1] for n in small]
        rq = _slot(modsx, ctx, q)
        parts = [_slot(modsx, ctx, x, seed=i) for i, x in enumerate(trains)]
        before = ctx.hamming_group_counters()
        got = ctx.rep_match_group_hamming(rq, parts, distance_threshold=ALL)
        assert _delta(ctx, before) == dict(launch_sets=1, problems=4, rows_packed=0, match_pack_launches=0)
        nn2 = HM.knn2(q, t)
        HM.check_planted(nn2, info)
        assert tuple(nn2[HM.PLANT["copies"]]) == (T - 1, 2, T, 2) and tuple(nn2[6]) == (start - 1, 2, start, 2)
        HM.same_tents(got[0], HM.tentatives(nn2, ALL))
        for g, x in zip(got[1:], trains[1:]):
            HM.same_tents(g, HM.match(q, x, ALL))
        # the other rotation: the big partner last, and cut by a threshold
        got = ctx.rep_match_group_hamming(rq, parts[1:] + parts[:1], distance_threshold=HM.MAX_DISTANCE)
        ref = HM.tentatives(nn2, HM.MAX_DISTANCE)
        assert 0 < len(ref) < n1
        HM.same_tents(got[3], ref)
        _free(rq, *parts)


def test_neighbours_are_partner_local(modsx, ctx):
    with _Gpu():
        nbytes, n2 = 32, BC.tile_len(32) + 1
        q = HM.random_rows(64, 2, nbytes, 31)[0]
        trains = [HM.random_rows(2, n2, nbytes, 90 + g)[1] for g in range(4)]
        for g in range(3):
            trains[g + 1][0] = q[g]                               # an exact copy of query g is the FIRST row of partner g + 1
        for g in range(4):
            assert HM.distances(q, trains[g])[np.arange(64) != (g - 1 if g else -1)].min() >= 3
        rq = _slot(modsx, ctx, q)
        parts = [_slot(modsx, ctx, t, seed=g) for g, t in enumerate(trains)]
        got = ctx.rep_match_group_hamming(rq, parts, distance_threshold=ALL)
        for g in range(4):
            HM.same_tents(got[g], HM.match(q, trains[g], ALL))
            if g < 3:
                assert got[g]["d1"][g] >= 3                       # partner g holds nothing closer than 3 to query g: the copy next door is not its
                assert got[g + 1]["t0"][g] == 0 and got[g + 1]["d1"][g] == 0
        _free(rq, *parts)


# ---- 5. match_reps -----------------------------------------------------------------------------------------------------------------
def _same_pair_result(got, ref):
    for k in ("n_regions", "n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples", "ransac_lo"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    HM.same_tents(got["tentatives"], ref["tentatives"])
    assert np.array_equal(got["ransac_inlier"], ref["ransac_inlier"]) and np.array_equal(got["verified"], ref["verified"])
    assert got["H"].tobytes() == ref["H"].tobytes()


def _tail(lib, l1, l2, tent, par, seed):
    """DuplicateFiltering (key = ratio) + LORANSACFiltering on the concatenated lists: the existing pair tail"""
    pts = np.stack([l1["reproj_kp"]["x"][tent["q"]], l1["reproj_kp"]["y"][tent["q"]],
                    l2["reproj_kp"]["x"][tent["t0"]], l2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = lib.duplicate_filtering(pts, tent["ratio"], par.duplicateDist, True)
    sel = order[keep]
    tu, pu = tent[sel], pts[sel]
    rr = lib.loransac_h(pu, laf_of(l1, tu["q"]), laf_of(l2, tu["t0"]), err_threshold=par.err_threshold, confidence=par.confidence,
                        max_samples=par.max_samples, lo=par.localOptimization, hlaf_coef=par.HLAFCoef, sym_check=par.doSymmCheck,
                        seed=seed, error_type=par.errorType)
    return tu, rr


THR = 40.0
RS, SURF = 1, 12


def _class_lists(modsx, ctx, ra, rb, classes, par):
    """the per-class region lists and tentatives (from the per-class taps) in the order of rep_class_order, re-based"""
    l1, l2, tents = [], [], []
    for det, typ in sorted(classes, key=lambda k: modsx.rep_class_order(*k)):
        if typ >= 16:
            g1, g2 = ra.regions_bin(det, typ, want_desc=False), rb.regions_bin(det, typ, want_desc=False)
            t = ctx.rep_match_hamming(ra, rb, det, typ, THR) if len(g1) and len(g2) else np.zeros(0, modsx.TENT)
        elif typ >= 8:
            g1, g2 = ra.class_f32(det, typ)[0], rb.class_f32(det, typ)[0]
            t = ctx.rep_match_fginn_f32(ra, rb, det, typ, par.match_ratio, par.contradDist, par.nn)
        else:
            g1, g2 = ra.regions(det, typ, want_desc=False), rb.regions(det, typ, want_desc=False)
            t = ctx.rep_match_fginn(ra, rb, det, typ, par.match_ratio, par.contradDist, par.nn)
        t = t.copy()
        t["q"] += sum(len(x) for x in l1)
        for f in ("t0", "tj", "t1"):
            t[f] = np.where(t[f] >= 0, t[f] + sum(len(x) for x in l2), t[f])
        l1.append(g1); l2.append(g2); tents.append(t)
    return np.concatenate(l1), np.concatenate(l2), tents


def _three_class_rep(modsx, ctx, regs, bits, with_bin=True):
    """ORB x ORB rows, HessianAffine RootSIFT descriptors and SURF x SURF float rows that keep the neighbourhoods of the bits"""
    rep = modsx.Rep(ctx)
    n = len(regs)
    sift = np.repeat(np.unpackbits(bits[:, :16], axis=1), 1, axis=1).astype(np.uint8) * 90 + (np.arange(128) % 7).astype(np.uint8)
    surf = (np.unpackbits(bits[:, 16:24], axis=1).astype(np.float32) - np.float32(0.5)) * np.float32(0.37)
    rep.append(regs[:n - 40], sift[:n - 40], HES, RS)             # the three classes have lists of different lengths
    rep.append_f32(regs[:n - 90], surf[:n - 90], SURFDET, SURF)
    if with_bin:
        rep.append_bin(regs, bits, ORBDET, ORB)
    return rep


def test_match_reps_three_kinds_of_classes_five_partners(modsx, ctx):
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=6)
        r1, d1, _, _ = BC.planted_pair(modsx, seed=5)
        ra = _three_class_rep(modsx, ctx, r1, d1)
        partners = []
        for i in range(5):
            _, _, r2, d2 = BC.planted_pair(modsx, seed=5 if i in (0, 2, 4) else 11 + i)      # seed 5: the partner of r1
            n = (500, 260, 500, 131, 500)[i]
            partners.append(_three_class_rep(modsx, ctx, r2[:n], d2[:n], with_bin=i != 2))      # partner 2 lacks the binary class
        classes = [(HES, RS), (ORBDET, ORB), (SURFDET, SURF)]
        orders = [modsx.rep_class_order(*k) for k in classes]
        assert sorted(orders) != orders                           # listed in another order than they are concatenated in
        sel = [(d, t, THR if t >= 16 else par.match_ratio) for d, t in classes]
        before = ctx.hamming_group_counters()
        got = modsx.match_reps([ctx], ra, partners, par, sel)
        assert _delta(ctx, before) == dict(launch_sets=2, problems=4, rows_packed=0, match_pack_launches=0)      # two groups: 4 + 1
        nbin = 0
        for i, rb in enumerate(partners):
            l1, l2, tents = _class_lists(modsx, ctx, ra, rb, classes, par)
            tent = np.concatenate(tents)
            nbin += len(tents[0])                                 # names sort ORB < RootSIFT < SURF: the binary class comes first
            assert got[i]["n_regions"] == (len(l1), len(l2)) and got[i]["n_tentatives"] == len(tent), i
            tu, rr = _tail(modsx, l1, l2, tent, par, 6)
            assert got[i]["n_unique"] == len(tu)
            HM.same_tents(got[i]["tentatives"], tu)
            if i in (0, 2, 4):                                    # the partners related to ra: a model is found
                assert np.array_equal(got[i]["ransac_inlier"], rr["inl"]) and np.array_equal(got[i]["verified"], rr["keep"])
                assert got[i]["n_verified"] == rr["n"] > 100
                assert np.abs(normH(got[i]["H"]) - normH(rr["H"])).max() < 1e-4
        first = sorted(classes, key=lambda k: modsx.rep_class_order(*k))[0]
        assert first == (ORBDET, ORB) and nbin > 300 and got[0]["n_verified"] > 100
        assert len(partners[2].regions_bin(want_desc=False)) == 0 and got[2]["n_regions"][1] == 500 - 40 + 500 - 90
        _free(ra, *partners)


@pytest.mark.parametrize("use_f", [0, 1])
def test_match_reps_with_one_binary_class_equals_match_regions_hamming(modsx, ctx, use_f):
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=1, useF=1, LAFCoef=2.0, err_threshold=4.0) if use_f else \
            modsx.default_pair_params(ransac_seed=1)
        r1, d1, r2, d2 = BC.planted_pair(modsx, seed=8)
        d2[3] = d2[4] = d1[0]                                     # d1 = d2 = 0: a NaN ratio goes through DuplicateFiltering as it does there
        ref = ctx.match_regions_hamming(r1, d1, r2, d2, THR, par)
        assert ref["n_verified"] >= 150
        ra, rb = modsx.Rep(ctx), modsx.Rep(ctx)
        ra.append_bin(r1, d1, HES, FREAK); rb.append_bin(r2, d2, HES, FREAK)
        _same_pair_result(modsx.match_reps([ctx], ra, [rb], par, [(HES, FREAK, THR)])[0], ref)
        # n_classes == 0 leaves binary classes out: there is no distance threshold in the pair parameters
        none = modsx.match_reps([ctx], ra, [rb], par)[0]
        assert none["n_regions"] == (0, 0) and none["n_tentatives"] == 0 and none["n_verified"] == 0
        _free(ra, rb)


def test_a_selection_without_the_binary_class_gives_what_it_gave_before(modsx, ctx):
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=6)
        r1, d1, r2, d2 = BC.planted_pair(modsx, seed=5)
        ra, rb = _three_class_rep(modsx, ctx, r1, d1, with_bin=False), _three_class_rep(modsx, ctx, r2, d2, with_bin=False)
        sel = [(SURFDET, SURF, par.match_ratio), (HES, RS, par.match_ratio)]
        listed, every = modsx.match_reps([ctx], ra, [rb], par, sel)[0], modsx.match_reps([ctx], ra, [rb], par)[0]
        assert listed["n_verified"] > 50
        ra.append_bin(r1, d1, ORBDET, ORB); rb.append_bin(r2, d2, ORBDET, ORB)
        ra.append_bin(r1[:9], d1[:9, :7], MSER, BRISK)
        _same_pair_result(modsx.match_reps([ctx], ra, [rb], par, sel)[0], listed)
        _same_pair_result(modsx.match_reps([ctx], ra, [rb], par)[0], every)
        _free(ra, rb)


# ---- 6. counters -----------------------------------------------------------------------------------------------------------------------
def test_counters_book_launch_sets_problems_and_appended_rows(modsx, ctx):
    with _Gpu():
        q, t = HM.random_rows(40, 90, 32, 2)
        before = ctx.hamming_group_counters()
        rq = _slot(modsx, ctx, q)
        parts = [_slot(modsx, ctx, t[:n]) for n in (90, 0, 50, 2)]
        assert _delta(ctx, before) == dict(launch_sets=0, problems=0, rows_packed=40 + 90 + 50 + 2, match_pack_launches=0)
        before = ctx.hamming_group_counters()
        ctx.rep_match_group_hamming(rq, parts, distance_threshold=ALL)
        assert _delta(ctx, before) == dict(launch_sets=1, problems=3, rows_packed=0, match_pack_launches=0)
        before = ctx.hamming_group_counters()
        ctx.rep_match_group_hamming(rq, [parts[0], parts[2], parts[3], parts[0]], distance_threshold=ALL)
        assert _delta(ctx, before) == dict(launch_sets=1, problems=4, rows_packed=0, match_pack_launches=0)
        before = ctx.hamming_group_counters()
        ctx.match_hamming(q, t, ALL)                              # the single-problem entry packs both sides for every call
        assert _delta(ctx, before) == dict(launch_sets=0, problems=0, rows_packed=0, match_pack_launches=2)
        _free(rq, *parts)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_representations_as_they_were(modsx, ctx):
    with _Gpu():
        nbytes = 32
        q, t = HM.random_rows(65, 130, nbytes, 3)
        regs_q, regs_t = BC.regs_for(modsx, 65, 1), BC.regs_for(modsx, 130, 2)
        rq, rt, one, narrow, empty = modsx.Rep(ctx), modsx.Rep(ctx), modsx.Rep(ctx), modsx.Rep(ctx), modsx.Rep(ctx)
        rq.append_bin(regs_q, q); rt.append_bin(regs_t, t)
        one.append_bin(regs_t[:1], t[:1]); narrow.append_bin(regs_t[:9], t[:9, :31])
        ok = HM.match(q, t, ALL)
        par = modsx.default_pair_params(ransac_seed=1)

        def refused(fn, what=r".+"):
            with pytest.raises(RuntimeError, match=r"\(-1\): " + what):      # MODSX_ERR_ARG with a message
                fn()
            assert rq.count_bin() == 65 and rt.count_bin() == 130 and one.count_bin() == 1
            assert np.array_equal(rt.regions_bin()[1], t)
            HM.same_tents(ctx.rep_match_hamming(rq, rt, distance_threshold=ALL), ok)      # a following valid call succeeds

        # a train class of exactly one region: the tap, a group when any partner has one, match_reps when any partner has one
        refused(lambda: ctx.rep_match_hamming(rq, one, distance_threshold=ALL), r".*second neighbour")
        for group in ([one], [rt, one], [rt, empty, rt, one], [one, rt]):
            refused(lambda: ctx.rep_match_group_hamming(rq, group, distance_threshold=ALL), r".*second neighbour")
        refused(lambda: ctx.rep_match_hamming(empty, one, distance_threshold=ALL), r".*second neighbour")      # whatever n1 is
        refused(lambda: modsx.match_reps([ctx], rq, [rt, rt, rt, rt, rt, one], par, [(ORBDET, ORB, ALL)]), r".*second neighbour")
        # the threshold
        for thr in (0.0, -1.0, float("nan"), float("inf")):
            refused(lambda: ctx.rep_match_hamming(rq, rt, distance_threshold=thr), r".*distanceThreshold")
            refused(lambda: ctx.rep_match_group_hamming(rq, [rt, rt], distance_threshold=thr), r".*distanceThreshold")
            refused(lambda: modsx.match_reps([ctx], rq, [rt], par, [(ORBDET, ORB, thr)]), r".*distanceThreshold")
        # widths
        for nb in (0, 65):
            refused(lambda: rt.append_bin(regs_t[:4], np.zeros((4, nb), np.uint8)), r".*nbytes")
        keep, p = _dev(t[:4])
        refused(lambda: rt.append_bin_device(regs_t[:4], p, 65), r".*nbytes")
        refused(lambda: rt.append_bin_device(regs_t[:4], p, 31), r".*another width")
        refused(lambda: rt.append_bin(regs_t[:4], t[:4, :31]), r".*another width")
        refused(lambda: ctx.rep_match_hamming(rq, narrow, distance_threshold=ALL), r".*widths")
        refused(lambda: ctx.rep_match_group_hamming(rq, [rt, narrow], distance_threshold=ALL), r".*widths")
        refused(lambda: modsx.match_reps([ctx], rq, [rt, narrow], par, [(ORBDET, ORB, ALL)]), r".*widths")
        # pairs that name no binary class
        for det, typ in ((1, ORB), (2, ORB), (5, ORB), (7, BRISK), (-1, ORB), (ORBDET, 15), (ORBDET, 19), (ORBDET, 4), (HES, 1), (HES, 12)):
            refused(lambda: rt.append_bin(regs_t[:4], t[:4], det, typ))
            refused(lambda: rt.append_bin_device(regs_t[:4], p, nbytes, det, typ))
            refused(lambda: rt.regions_bin(det, typ))
            refused(lambda: ctx.rep_match_hamming(rq, rt, det, typ, ALL))
            refused(lambda: ctx.rep_match_group_hamming(rq, [rt], det, typ, ALL))
        for det, typ in ((1, ORB), (ORBDET, 15), (ORBDET, 19), (ORBDET, 1), (ORBDET, 12)):
            refused(lambda: modsx.match_reps([ctx], rq, [rt], par, [(det, typ, ALL)]))
        # G outside 1..4
        refused(lambda: ctx.rep_match_group_hamming(rq, [], distance_threshold=ALL))
        refused(lambda: ctx.rep_match_group_hamming(rq, [rt] * 5, distance_threshold=ALL))
        # more than 2 000 000 regions in a class: refused before anything is read
        L = modsx.lib()
        assert L.modsx_rep_append_bin(ctx.h, rt.h, ORBDET, ORB, regs_t.ctypes.data, t.ctypes.data, nbytes, 0, 2000001 - 130) == -1
        assert rt.count_bin() == 130
        # every entry that takes the types 0..3 alone, or 8..12, still refuses the new ones (and the ORB detector)
        refused(lambda: rt.append(regs_t[:4], np.zeros((4, 128), np.uint8), HES, ORB))
        refused(lambda: rt.append(regs_t[:4], np.zeros((4, 128), np.uint8), ORBDET, 1))
        refused(lambda: rt.append_f32(regs_t[:4], np.zeros((4, 64), np.float32), HES, ORB))
        refused(lambda: rt.append_f32(regs_t[:4], np.zeros((4, 64), np.float32), ORBDET, 12))
        refused(lambda: ctx.rep_match_fginn(rq, rt, HES, FREAK))
        refused(lambda: ctx.rep_match_fginn_f32(rq, rt, HES, BRISK))
        refused(lambda: ctx.rep_match_group_f32(rq, [rt], ORBDET, ORB))
        refused(lambda: rt.regions(ORBDET, ORB))
        refused(lambda: rt.class_f32(ORBDET, ORB))
        _free(rq, rt, one, narrow, empty)
