"""GPU: stored image representations (modsx_rep, engine_reps.hip) -- describe once, match against many.

What a representation holds is compared with the per-view loop's output; what matching two representations gives is compared
with modsx_match_ladder / modsx_match_pair_views on the same images field for field, and with the oracle-side ladder of
tests/common.py at the tolerances of the existing ladder tests; the pre-packed train side of the matcher is compared with
modsx_match_fginn_device on the same arrays over the case tables of tests/match_cases.py.

Fault latch: a HIP error met by any test of this module sets _FAULT; every later test then fails at once, before it touches the
GPU -- nothing is retried."""
import numpy as np
import pytest

from common import check_batch_statistics, need_ref, normH, oracle_ladder, same_records
from tests import match_cases as MC

pytestmark = pytest.mark.gpu

HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "hipmemcpy", "hipstream",
                   "hipgetlasterror", "unspecified launch failure", "queue error")
_FAULT = None
SEED = 6
B2_H = [[0.97, -0.06, 12], [0.05, 1.02, -7], [2e-5, -1e-5, 1]]
LADDER = (([1], 360.0, 0.8), ([1, 2], 360.0, 0.8), ([1, 2], 120.0, 0.85))      # the steps of test_iteration_ladder_matches_oracle


def _latch():
    if _FAULT is not None:
        pytest.fail("an earlier test of this module met a device error; nothing more is started on the GPU:\n%s" % _FAULT, pytrace=False)


class _Gpu(object):
    """the body of a test: a device error inside it ends the module's GPU work"""

    def __enter__(self):
        _latch()

    def __exit__(self, et, ev, tb):
        global _FAULT
        if ev is not None and isinstance(ev, RuntimeError) and any(m in str(ev).lower() for m in HIP_ERROR_MARKS):
            _FAULT = str(ev)[-1500:]
        return False


@pytest.fixture(scope="module")
def images(small_pair):
    from mods_amd import synthetic
    a, b, _ = small_pair
    return dict(a=a, b=b, blank=np.full((96, 128), 90, np.float32), unrelated=synthetic.blob_image(240, 320, 420, 778),
                b2=synthetic.warp_homography(synthetic.blob_image(240, 320, 420, 777), np.array(B2_H), seed=99))


@pytest.fixture(scope="module")
def ctxs(ctx, modsx):
    other = modsx.Context(0)
    yield [ctx, other]
    other.close()


@pytest.fixture(scope="module")
def dev(ctx, images):
    """the images in HBM, uploaded once"""
    up = {k: ctx.upload(v) for k, v in images.items()}
    yield up
    for im in up.values():
        im.free()


@pytest.fixture(scope="module")
def ladder(modsx, oracle):
    prev_o, prev_m, steps_o, steps_m = [], [], [], []
    for tilts, phi, ratio in LADDER:
        vo = oracle.set_vs_pars([1.0], tilts, phi, 0.2, 1, prev_o)
        vm = modsx.set_vs_pars([1.0], tilts, phi, 0.2, 1, prev_m)
        assert len(vo) == len(vm) and len(vo) > 0
        steps_o.append((vo, ratio)); steps_m.append((vm, ratio))
    assert [len(v) for v, _ in steps_m] == [1, 1, 2]
    return steps_o, steps_m


@pytest.fixture(scope="module")
def oracle_runs(oracle, images, ladder):
    """(partner, min_matches) -> (result, steps) of the oracle-side ladder of image a against the partner, computed once"""
    cache = {}

    def run(name, min_matches):
        if (name, min_matches) not in cache:
            cache[name, min_matches] = oracle_ladder(oracle, images["a"], images[name], ladder[0], min_matches, SEED, ori=(1.0, 41, 1, 0.8))
        return cache[name, min_matches]
    return run


def _same_pair_result(got, ref):
    for k in ("n_regions", "n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples", "ransac_lo"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert same_records(got["tentatives"], ref["tentatives"])
    assert np.array_equal(got["ransac_inlier"], ref["ransac_inlier"]) and np.array_equal(got["verified"], ref["verified"])
    assert got["H"].tobytes() == ref["H"].tobytes()


def _same_as_oracle(got, ref):
    assert got["n_regions"] == ref["n_regions"] and got["n_tentatives"] == ref["n_tentatives"]
    for f in ref["tent"].dtype.names:
        assert np.array_equal(got["tentatives"][f], ref["tent"][f]), f
    assert np.array_equal(got["ransac_inlier"], ref["rr"]["inl"]) and np.array_equal(got["verified"], ref["rr"]["keep"])
    assert np.abs(normH(got["H"]) - normH(ref["rr"]["H"])).max() < 1e-4


def _grow(rep, img, steps, par, upto, done=0):
    for st in steps[done:upto]:
        rep.add_views(img, st[0], par, detector=st[2] if len(st) > 2 else 0, descs=st[3] if len(st) > 3 else None)
    return rep


# ---- 1. content ------------------------------------------------------------------------------------------------------------------
def test_representation_holds_the_view_loops_regions_and_descriptors(ctx, modsx, dev, ladder):
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=SEED)
        rep = modsx.Rep(ctx)
        assert rep.count() == 0
        want_r, want_d = np.zeros(0, modsx.REGION), np.zeros((0, 128), np.uint8)
        for views, _ in ladder[1]:
            r, d = ctx.detect_describe_views(dev["a"], views, par)
            r = r.copy()
            r["id"] += len(want_r); r["parent_id"] += len(want_r)          # AddRegionsToList
            want_r, want_d = np.concatenate([want_r, r]), np.concatenate([want_d, d.astype(np.uint8)])
            assert np.array_equal(d, d.astype(np.uint8).astype(np.float32))
            assert rep.add_views(dev["a"], views, par) == len(r)
            got_r, got_d = rep.regions()
            assert same_records(got_r, want_r) and np.array_equal(got_d, want_d)
            for det, typ in ((0, 0), (0, 2), (0, 3), (3, 1)):
                assert rep.count(det, typ) == 0
        assert rep.count() == 473
        rep.free()


# ---- 2. pair equivalence ---------------------------------------------------------------------------------------------------------
def test_match_reps_equals_the_ladder_and_the_oracle(ctx, modsx, oracle, dev, ladder, oracle_runs):
    need_ref(oracle)
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=SEED)
        steps_m = ladder[1]
        ra, rb = modsx.Rep(ctx), modsx.Rep(ctx)
        done = 0
        for k, classes in ((1, None), (3, [(0, 1, 0.85)])):     # None: par's ratio, 0.8; after step 3 the class was last matched with 0.85
            _grow(ra, dev["a"], steps_m, par, k, done); _grow(rb, dev["b"], steps_m, par, k, done)
            done = k
            got = modsx.match_reps([ctx], ra, [rb], par, classes)[0]
            ref, n = ctx.match_ladder(dev["a"], dev["b"], steps_m[:k], par, min_matches=10 ** 6)
            assert n == k
            _same_pair_result(got, ref)
            # min_matches 10 stops the oracle-side ladder after one step (88 verified), 10 ** 6 lets it run all three
            oref, odone = oracle_runs("b", 10 if k == 1 else 10 ** 6)
            assert odone == k
            _same_as_oracle(got, oref)
            if k == 1:
                assert got["n_regions"] == (144, 129) and got["n_tentatives"] == 92 and got["n_verified"] == 88
            else:
                assert got["n_verified"] == 178
        ra.free(); rb.free()


def _wxbs_params(modsx, seed, useF):
    """config_iter_mods_cviu_wxbs.ini as test_gpu_views._wxbs_ladder_params states it, 300 / 120 regions"""
    par = modsx.default_pair_params(
        mode=4, threshold=5.3333, reg_number=300, ori_mrSize=5.1962, ori_maxAngles=5, ori_threshold=0.8,
        desc_mrSize=5.1962, desc_photoNorm=1, desc_maxBinValue=0.2, contradDist=10.0, duplicateDist=3.0,
        err_threshold=4.0, confidence=0.99, max_samples=1000000, localOptimization=1, LAFCoef=3.0, HLAFCoef=13.0,
        doSymmCheck=1, useF=useF, ransac_seed=seed)
    par.mser.mode = 2
    par.mser.reg_number = 120
    return par


@pytest.mark.parametrize("useF", [0, 1])
def test_match_reps_two_descriptor_classes_equals_the_ladder(ctx, modsx, dev, useF):
    """[MSER2] of the WxBS ladder: RootSIFT (0.85) and HalfRootSIFT (0.8) on one Half-folded oriented list; H and F"""
    with _Gpu():
        descs = [(1, 0.85), (3, 0.8)]
        views = modsx.set_vs_pars([1, 0.25, 0.125], [1], 360.0, 0.8, 1, [])
        assert len(views) == 3
        par = _wxbs_params(modsx, 7, useF)
        step = (views, 0.0, 3, descs)
        ra, rb = _grow(modsx.Rep(ctx), dev["a"], [step], par, 1), _grow(modsx.Rep(ctx), dev["b"], [step], par, 1)
        assert ra.count(3, 1) == ra.count(3, 3) > 50 and ra.count(0, 1) == 0
        ref, _ = ctx.match_ladder(dev["a"], dev["b"], [step], par, min_matches=10 ** 6)
        if useF:      # the ratios through the parameter block's descriptor list
            par2 = _wxbs_params(modsx, 7, useF)
            par2.n_desc = 2
            for i, (t, r) in enumerate(descs):
                par2.desc_types[i], par2.desc_ratios[i] = t, r
            got = modsx.match_reps([ctx], ra, [rb], par2)[0]
        else:         # ... and as explicit classes
            got = modsx.match_reps([ctx], ra, [rb], par, [(3, 1, 0.85), (3, 3, 0.8)])[0]
        _same_pair_result(got, ref)
        assert got["n_verified"] > 10 and got["n_regions"][0] == 2 * ra.count(3, 1)
        ra.free(); rb.free()


def test_match_reps_mixed_detectors_equals_the_ladder(ctx, modsx, dev):
    """the four steps of test_mixed_mser_hessaff_ladder_matches_oracle: MSER, HessianAffine, MSER, HessianAffine"""
    with _Gpu():
        prev, steps = {0: [], 3: []}, []
        for det, tilts, phi, sigma, ratio in ((3, [1], 360.0, 0.8, 0.85), (0, [1], 360.0, 0.2, 0.8), (3, [1, 3], 360.0, 0.8, 0.8),
                                              (0, [1, 2], 360.0, 0.2, 0.8)):
            steps.append((modsx.set_vs_pars([1.0], tilts, phi, sigma, 1, prev[det]), ratio, det))
        par = modsx.default_pair_params(ransac_seed=8)
        ra, rb = _grow(modsx.Rep(ctx), dev["a"], steps, par, 4), _grow(modsx.Rep(ctx), dev["b"], steps, par, 4)
        ref, n = ctx.match_ladder(dev["a"], dev["b"], steps, par, min_matches=10 ** 6)
        assert n == 4
        got = modsx.match_reps([ctx], ra, [rb], par, [(3, 1, 0.8), (0, 1, 0.8)])[0]     # the last ratio of each class
        _same_pair_result(got, ref)
        n1 = ra.count(0, 1)
        assert n1 > 0 and ra.count(3, 1) > 0 and got["n_regions"][0] == n1 + ra.count(3, 1)
        assert (got["tentatives"]["q"] < n1).any() and (got["tentatives"]["q"] >= n1).any()     # HessianAffine first, then MSER
        ra.free(); rb.free()


# ---- 3. many partners ------------------------------------------------------------------------------------------------------------
def test_match_reps_many_partners_equal_single_pairs(ctxs, modsx, dev):
    """six partners over two contexts: two groups (MATCH_MAXB = 4), an empty problem inside the first"""
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=SEED)
        views = modsx.set_vs_pars([1.0], [1, 2], 360.0, 0.2, 1, [])
        names = ["b", "blank", "unrelated", "b2", "a", "b"]
        ra = modsx.Rep(ctxs[0])
        ra.add_views(dev["a"], views, par)
        reps = []
        for i, nm in enumerate(names):       # any context of the device may build a representation
            r = modsx.Rep(ctxs[0])
            r.add_views(dev[nm], views, par, ctx=ctxs[i % 2])
            reps.append(r)
        assert reps[1].count() == 0
        got = modsx.match_reps(ctxs, ra, reps, par)
        check_batch_statistics(modsx, 2, 6, 4)
        light = modsx.match_reps(ctxs, ra, reps, par, arrays=False)
        check_batch_statistics(modsx, 2, 6, 4)
        assert len(got) == 6
        for i, nm in enumerate(names):
            ref = ctxs[0].match_pair_views(dev["a"], dev[nm], views, par)
            _same_pair_result(got[i], ref)
            assert light[i]["n_verified"] == ref["n_verified"] and light[i]["H"].tobytes() == ref["H"].tobytes()
        assert got[1]["n_regions"] == (ra.count(), 0) and got[1]["n_tentatives"] == 0 and got[1]["n_verified"] == 0
        assert (got[1]["H"] == -1).all()
        assert got[0]["n_verified"] > 50 and got[3]["n_verified"] > 50 and got[4]["n_verified"] > 100 and got[2]["n_verified"] == 0
        assert modsx.match_reps(ctxs, ra, [], par) == []
        for r in reps + [ra]:
            r.free()


# ---- 4. the pre-packed train side of the matcher ---------------------------------------------------------------------------------
def _regs_at(modsx, pos):
    r = np.zeros(len(pos), modsx.REGION)
    r["reproj_kp"]["x"], r["reproj_kp"]["y"] = pos[:, 0], pos[:, 1]
    return r


def _u8(a):
    return np.ascontiguousarray(a, np.float32).astype(np.uint8)


def _device_ref(ctx, d1, d2, pos2, p):
    import torch
    t1, t2 = torch.from_numpy(_u8(d1)).cuda(), torch.from_numpy(_u8(d2)).cuda()
    torch.cuda.synchronize()
    return ctx.match_fginn_device(t1.data_ptr(), len(d1), t2.data_ptr(), len(d2), np.ascontiguousarray(pos2), *p)


@pytest.mark.parametrize("case", MC.small_cases() + (MC.big_n2_case(),), ids=lambda c: c.name)
def test_prepacked_trains_equal_the_per_call_pack(ctx, modsx, case):
    with _Gpu():
        n1, n2 = len(case.d1), len(case.d2)
        r1, r2 = modsx.Rep(ctx), modsx.Rep(ctx)
        r1.append(np.zeros(n1, modsx.REGION), case.d1)                       # f32 holding integers
        # two appends: 70 000 trains go in as 40 000 + 30 000, across the 65 536-row first capacity (re-allocation, re-pack)
        cut = 40000 if n2 > 65536 else n2 - n2 // 3
        regs2 = _regs_at(modsx, case.pos2)
        assert r2.append(regs2[:cut], _u8(case.d2[:cut])) == cut             # u8
        assert r2.append(regs2[cut:], _u8(case.d2[cut:])) == n2 - cut
        assert r2.count() == n2
        total = 0
        for p in case.params:
            ref = _device_ref(ctx, case.d1, case.d2, case.pos2, p)
            got = ctx.rep_match_fginn(r1, r2, 0, 1, *p)
            assert MC.same_tentatives(got, ref), (case.name, p, len(got), len(ref))
            total += len(ref)
        assert total >= min(5, n1), "nothing was compared"
        if n2 > 65536:
            gr, gd = r2.regions()
            assert np.array_equal(gd, _u8(case.d2)) and np.array_equal(gr["reproj_kp"]["x"], case.pos2[:, 0])
        r1.free(); r2.free()


def test_a_grown_class_is_repacked(ctx, modsx):
    """matched, grown by 33 trains that are the new nearest neighbours of 33 queries, matched again: a stale pack gives the old answer"""
    with _Gpu():
        case = MC.ragged_block_cases()[0]
        p = case.params[0]
        r1, r2 = modsx.Rep(ctx), modsx.Rep(ctx)
        r1.append(np.zeros(len(case.d1), modsx.REGION), case.d1)
        r2.append(_regs_at(modsx, case.pos2), case.d2)
        before = ctx.rep_match_fginn(r1, r2, 0, 1, *p)
        assert MC.same_tentatives(before, _device_ref(ctx, case.d1, case.d2, case.pos2, p))
        k = min(33, len(case.d1))
        more = case.d1[:k].copy()                                            # exact copies of the first queries: d0 = 0 there
        pos_more = np.random.RandomState(3).uniform(0, 50, (k, 2))
        r2.append(_regs_at(modsx, pos_more), more)
        d2, pos2 = np.concatenate([case.d2, more]), np.concatenate([case.pos2, pos_more])
        ref = _device_ref(ctx, case.d1, d2, pos2, p)
        after = ctx.rep_match_fginn(r1, r2, 0, 1, *p)
        assert MC.same_tentatives(after, ref)
        assert not MC.same_tentatives(after, before) and (after["t0"] >= len(case.d2)).any()
        r1.free(); r2.free()


# ---- 5. one against many over the ladder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("partners,min_matches,want_done", [(("unrelated", "b", "b2"), 10, 1), (("unrelated", "b"), 100, None),
                                                            (("unrelated",), 10, 3)], ids=["any_reaches_10", "b_reaches_100", "none"])
def test_one_to_many_stops_when_any_partner_has_enough(ctxs, modsx, oracle, dev, ladder, oracle_runs, partners, min_matches, want_done):
    need_ref(oracle)
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=SEED)
        steps_m = ladder[1]
        # GetAtLeastOneImageMatch: the loop ends with the first partner that has enough -- the smallest step count over the
        # partners' own ladders (a ladder that never has enough runs all steps)
        expect = min(oracle_runs(nm, min_matches)[1] for nm in partners)
        if want_done is not None:
            assert expect == want_done
        got, done = modsx.match_one_to_many(ctxs, dev["a"], [dev[nm] for nm in partners], steps_m, par, min_matches=min_matches)
        assert done == expect and len(got) == len(partners)
        for nm, g in zip(partners, got):
            ref, n = ctxs[0].match_ladder(dev["a"], dev[nm], steps_m[:done], par, min_matches=10 ** 6)
            assert n == done
            _same_pair_result(g, ref)
        if done < len(steps_m):
            assert any(g["n_verified"] >= min_matches for g in got)
        if partners == ("unrelated",):
            assert got[0]["n_verified"] == 0 and got[0]["n_tentatives"] == 42


def test_a_refused_ladder_step_fails_the_whole_one_to_many_call(ctxs, modsx, dev, ladder):
    """One ladder step whose second view the host planner refuses (views_plan.cpp, before any kernel of that view set is launched),
    two partners over two contexts: the call raises the planner's error.  The same contexts then run the good ladder and give
    what the per-pair ladder gives (b or b2 has ten matches after the first step: any_reaches_10 above)."""
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=SEED)
        steps_m = ladder[1]
        partners = ("b", "b2")
        bad = [([steps_m[0][0][0], modsx.make_view(1e9, 0.0, 1.0, 0.2, 1)], 0.8)]
        with pytest.raises(RuntimeError, match="degenerate"):
            modsx.match_one_to_many(ctxs, dev["a"], [dev[nm] for nm in partners], bad, par, min_matches=10)
        got, done = modsx.match_one_to_many(ctxs, dev["a"], [dev[nm] for nm in partners], steps_m, par, min_matches=10)
        check_batch_statistics(modsx, 2, 2, 4)
        assert done == 1 and len(got) == 2
        for nm, g in zip(partners, got):
            ref, n = ctxs[0].match_ladder(dev["a"], dev[nm], steps_m[:done], par, min_matches=10 ** 6)
            assert n == done
            _same_pair_result(g, ref)
        assert any(g["n_verified"] >= 10 for g in got)


# ---- 6. database -----------------------------------------------------------------------------------------------------------------
def test_match_reps_with_a_database_equals_single_pairs(ctxs, modsx, dev):
    with _Gpu():
        par = modsx.default_pair_params(ransac_seed=SEED)
        views = modsx.set_vs_pars([1.0], [1, 2], 360.0, 0.2, 1, [])
        ra = modsx.Rep(ctxs[0])
        ra.add_views(dev["a"], views, par)
        reps = []
        for nm in ("b", "b2"):
            reps.append(modsx.Rep(ctxs[0]))
            reps[-1].add_views(dev[nm], views, par)
        # 4 096 seeded rows: near-copies of every other query descriptor (they reject or re-rate records), random rows for the rest
        rs = np.random.RandomState(11)
        qd = ra.regions()[1].astype(np.int64)
        near = np.clip(qd[::2] + rs.randint(-3, 4, qd[::2].shape), 0, 255)
        rows = np.concatenate([near, rs.randint(0, 60, (4096 - len(near), 128))]).astype(np.uint8)
        assert rows.shape == (4096, 128)
        plain = modsx.match_reps(ctxs, ra, reps, par)
        db = ctxs[0].db_create(rows)
        for c in ctxs:
            c.set_fginn_db(db)
        try:
            got = modsx.match_reps(ctxs, ra, reps, par)
            for g, nm in zip(got, ("b", "b2")):
                _same_pair_result(g, ctxs[0].match_pair_views(dev["a"], dev[nm], views, par))
            assert got[0]["n_tentatives"] < plain[0]["n_tentatives"] and got[1]["n_tentatives"] < plain[1]["n_tentatives"]
            assert got[0]["n_tentatives"] > 10
        finally:
            for c in ctxs:
                c.set_fginn_db(None)
        db.free()
        for r in reps + [ra]:
            r.free()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(ctxs, modsx):
    with _Gpu():
        par = modsx.default_pair_params()
        rep, other = modsx.Rep(ctxs[0]), modsx.Rep(ctxs[0])
        d = np.full((4, 128), 7.0, np.float32)
        d[2, 5] = 7.5
        with pytest.raises(RuntimeError, match=r"\(-1\): .*integers 0\.\.255"):
            rep.append(np.zeros(4, modsx.REGION), d)
        assert rep.count() == 0
        with pytest.raises(RuntimeError, match=r"\(-1\): .*context"):
            modsx.match_reps([], rep, [other], par)
        db = ctxs[0].db_create(np.zeros((8, 128), np.uint8))
        ctxs[0].set_fginn_db(db)
        try:
            with pytest.raises(RuntimeError, match=r"\(-1\): .*same descriptor database"):
                modsx.match_reps(ctxs, rep, [other], par)
        finally:
            ctxs[0].set_fginn_db(None)
        db.free()
        # two empty representations: the zeroed result with H = -1
        got = modsx.match_reps(ctxs, rep, [other], par)[0]
        assert got["n_regions"] == (0, 0) and got["n_tentatives"] == 0 and got["n_verified"] == 0 and (got["H"] == -1).all()
        rep.free(); other.free()
