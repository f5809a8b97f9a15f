"""GPU: the float descriptor classes of stored representations (engine_reps_f32.hip) and the grouped f32 search
(kernels_fginn32.hip k_f32g_*).  Expected records come from oracle.pyoracle.match_fginn and from the single-problem entries
(Context.match_fginn_f32, match_regions_f32, describe_regions_*), never from the code under test; the inputs are those of
tests/fginn32_cases.py, whose reach tests/test_fginn32_cases_cpu.py proves on the CPU.

Fault latch: a HIP error met by any test of this module sets _FAULT; every later test then fails at once, before it touches the
GPU -- nothing is retried."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fginn32_cases as FC
from common import laf_of, need_ref, normH, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "reps_f32_child.py")
CHILD_TIMEOUT_S = 120          # import + context creation + one call, as for tests/patchdesc_batch_child.py
HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "hipmemcpy", "hipstream",
                   "hipgetlasterror", "unspecified launch failure", "queue error")
_FAULT = None
HES, MSER, SURFDET = 0, 3, 6
CAFFE, DAISY, LIOP, MROGH, SURF = 8, 9, 10, 11, 12
TYPE_OF_DIM = {64: SURF, 144: LIOP, 200: DAISY, 192: MROGH}      # the other widths go into CAFFE


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


def _regs_at(modsx, pos):
    pos = np.asarray(pos, np.float64).reshape(-1, 2)
    r = np.zeros(len(pos), modsx.REGION)
    r["id"] = np.arange(len(r))
    r["reproj_kp"]["x"], r["reproj_kp"]["y"] = pos[:, 0], pos[:, 1]
    return r


def _slot(modsx, ctx, rows, pos=None, det=HES, typ=None):
    """a fresh representation whose one float class holds these rows (at these positions)"""
    rows = np.ascontiguousarray(rows, np.float32)
    typ = TYPE_OF_DIM.get(rows.shape[1], CAFFE) if typ is None else typ
    rep = modsx.Rep(ctx)
    regs = _regs_at(modsx, np.zeros((len(rows), 2)) if pos is None else pos)
    assert rep.append_f32(regs, rows, det, typ) == len(rows)
    return rep, typ


def _stored(modsx, ctx, c, nn, n1=None, n2=None, det=HES):
    q = c["q"] if n1 is None else c["q"][:n1]
    t, pos = (c["t"], c["pos"]) if n2 is None else (c["t"][:n2], c["pos"][:n2])
    r1, typ = _slot(modsx, ctx, q, det=det)
    r2, _ = _slot(modsx, ctx, t, pos, det=det)
    try:
        return ctx.rep_match_fginn_f32(r1, r2, det, typ, c["ratio"], c["cd"], nn)
    finally:
        r1.free(); r2.free()


def _ref(oracle, c, nn, n2=None):
    t, pos = (c["t"], c["pos"]) if n2 is None else (c["t"][:n2], c["pos"][:n2])
    return oracle.match_fginn(c["q"], t, pos, c["ratio"], c["cd"], nn)


# ---- 1. the stored form equals the per-call pack ---------------------------------------------------------------------------------
def _planted(modsx, name):
    if name == "tie_case":
        T = modsx.fginn32_geometry(70, 1000, 128)["tile"]
        return FC.tie_case(modsx.fginn32_geometry(70, FC.TIE_TILES * T - 2, 128))
    return getattr(FC, name)()


@pytest.mark.parametrize("name", ["walk_case", "tie_case", "short_case", "tiny_case", "threshold_case", "subnormal_case"])
def test_stored_form_equals_the_per_call_pack_on_the_planted_cases(modsx, oracle, ctx, name):
    with _Gpu():
        c = _planted(modsx, name)
        total = 0
        for nn in (2, 4, 50):
            ref = _ref(oracle, c, nn)
            FC.same_tents(_stored(modsx, ctx, c, nn), ref)
            FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], nn), ref)
            FC.same_tents(_stored(modsx, ctx, c, nn, det=SURFDET if nn == 4 else MSER), ref)      # the other detectors' slots
            total += len(ref)
        assert total > 0 or name in ("short_case", "tiny_case")


@pytest.mark.parametrize("dim", [64, 144, 200, 128])
def test_stored_form_at_sizes_around_workgroup_and_tile(modsx, oracle, ctx, dim):
    with _Gpu():
        T = modsx.fginn32_geometry(257, 1000, dim)["tile"]
        c = FC.random_case(257, 2 * T + 1, dim, 300 + dim, noise=0.9)
        q1, typ = _slot(modsx, ctx, c["q"][:1])
        reps_q = {1: q1}
        for n1 in (255, 256, 257):
            reps_q[n1] = _slot(modsx, ctx, c["q"][:n1])[0]
        compared = 0
        for n2 in (1, 3, T - 1, T, T + 1, 2 * T + 1):
            rt, _ = _slot(modsx, ctx, c["t"][:n2], c["pos"][:n2])
            for nn in (2, 4, 50):
                ref = _ref(oracle, c, nn, n2)
                FC.same_tents(ctx.match_fginn_f32(c["q"], c["t"][:n2], c["pos"][:n2], c["ratio"], c["cd"], nn), ref)
                for n1, rq in reps_q.items():
                    FC.same_tents(ctx.rep_match_fginn_f32(rq, rt, HES, typ, c["ratio"], c["cd"], nn), ref[ref["q"] < n1])
                compared += len(ref)
            rt.free()
        assert compared > 60
        for r in reps_q.values():
            r.free()


# ---- 2. groups -------------------------------------------------------------------------------------------------------------------
def _delta(ctx, before):
    now = ctx.fginn32_group_counters()
    return {k: now[k] - before[k] for k in now}


def test_groups_equal_the_single_calls_partner_by_partner(modsx, oracle, ctx):
    with _Gpu():
        dim = 144
        T = modsx.fginn32_geometry(257, 1000, dim)["tile"]
        sizes = [2 * T + 1, 0, 3, T]
        c = FC.random_case(257, sum(sizes), dim, 40, noise=0.9)      # the queries' near trains are dealt over the partners
        q, ends = c["q"], np.cumsum([0] + sizes)
        cut = [(c["t"][a:b], c["pos"][a:b]) for a, b in zip(ends, ends[1:])]
        rq, typ = _slot(modsx, ctx, q)
        parts = [_slot(modsx, ctx, t, p, typ=typ)[0] for t, p in cut]
        refs = [oracle.match_fginn(q, t, p, FC.RATIO, FC.CD, 50) for t, p in cut]
        assert len(refs[0]) > 20 and len(refs[1]) == 0 and len(refs[3]) > 5
        for order in ([0], [1], [0, 1], [1, 0], [2, 3, 0], [3, 2, 1], [0, 1, 2, 3], [3, 0, 2, 0]):
            before = ctx.fginn32_group_counters()
            got = ctx.rep_match_group_f32(rq, [parts[i] for i in order], HES, typ, FC.RATIO, FC.CD, 50)
            d = _delta(ctx, before)
            live = sum(1 for i in order if sizes[i] > 0)
            assert d["launch_sets"] == (1 if live else 0) and d["problems"] == live and d["resolve_launches"] <= 1, (order, d)
            assert len(got) == len(order)
            for g, i in zip(got, order):
                FC.same_tents(g, refs[i])
                FC.same_tents(g, ctx.rep_match_fginn_f32(rq, parts[i], HES, typ, FC.RATIO, FC.CD, 50))
        # an all-empty group and an empty query slot: no launch, no record
        empty = modsx.Rep(ctx)
        before = ctx.fginn32_group_counters()
        assert [len(g) for g in ctx.rep_match_group_f32(rq, [parts[1], empty, parts[1]], HES, typ, FC.RATIO, FC.CD, 50)] == [0, 0, 0]
        assert [len(g) for g in ctx.rep_match_group_f32(empty, [parts[0], parts[3]], HES, typ, FC.RATIO, FC.CD, 50)] == [0, 0]
        assert _delta(ctx, before) == dict(launch_sets=0, problems=0, resolve_queries=0, resolve_launches=0)
        for r in parts + [rq, empty]:
            r.free()


# ---- 3. no leakage between problems ------------------------------------------------------------------------------------------------
def test_neighbours_are_partner_local_and_padding_is_never_one(modsx, oracle, ctx):
    with _Gpu():
        dim = 128
        T = modsx.fginn32_geometry(64, 1000, dim)["tile"]
        n2 = T + 1                                               # T - 1 zero rows follow in the last tile
        rs = np.random.RandomState(9)
        q = (rs.randn(64, dim) * 3).astype(np.float32)
        q[1] = 0                                                 # a query that equals every padding row
        trains, poss = [], []
        for g in range(4):
            t = (rs.randn(n2, dim) * 3 + 1).astype(np.float32)
            trains.append(t); poss.append(rs.uniform(0, 20, (n2, 2)))
        for g in range(3):                                       # query 0 twice: last row of partner g, first row of partner g + 1
            trains[g][n2 - 1] = q[0]
            trains[g + 1][0] = q[0]
        rq, typ = _slot(modsx, ctx, q)
        parts = [_slot(modsx, ctx, t, p)[0] for t, p in zip(trains, poss)]
        got = ctx.rep_match_group_f32(rq, parts, HES, typ, FC.RATIO, FC.CD, 50)
        for g in range(4):
            ref = oracle.match_fginn(q, trains[g], poss[g], FC.RATIO, FC.CD, 50)
            FC.same_tents(got[g], ref)
            for f in ("t0", "tj", "t1"):
                assert (got[g][f] < n2).all() and (got[g][f] >= 0).all()
            r0 = got[g][got[g]["q"] == 0]
            assert len(r0) == 1 and r0["d1"][0] == 0.0
            # the duplicates of partner g are its nearest ones, at their local indices, whatever the neighbours hold there
            assert r0["t0"][0] == (n2 - 1 if g == 0 else 0) and (g in (0, 3) or r0["t1"][0] == n2 - 1)
            assert (got[g]["q"] == 1).sum() == (ref["q"] == 1).sum()
        # one train: every query has exactly one key, the walk runs out of trains at j = 1 -- a padding row taken for a train
        # would be the zero query's nearest neighbour at distance 0 and the real row would then pass the ratio test
        one, _ = _slot(modsx, ctx, trains[0][:1], poss[0][:1])
        assert len(oracle.match_fginn(q, trains[0][:1], poss[0][:1], FC.RATIO, FC.CD, 50)) == 0
        assert [len(g) for g in ctx.rep_match_group_f32(rq, [one, parts[0], one], HES, typ, FC.RATIO, FC.CD, 50)] == [0, len(got[0]), 0]
        for r in parts + [rq, one]:
            r.free()


# ---- 4. open walks in several problems of one group ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nn", [2, 4, 50])
def test_open_walks_of_two_problems_share_one_resolve_launch(modsx, oracle, ctx, nn):
    with _Gpu():
        a, b = FC.walk_case(seed=3), FC.walk_case(seed=12)       # the same clusters, the trains in another order
        assert np.array_equal(a["q"], b["q"]) and not np.array_equal(a["t"], b["t"])
        mid = FC.random_case(len(a["q"]), 70, 128, 5)
        rq, typ = _slot(modsx, ctx, a["q"])
        parts = [_slot(modsx, ctx, c["t"], c["pos"])[0] for c in (a, mid, b)]
        stages = []
        for c in (a, mid, b):
            ia, da = oracle.knn_linear(a["q"], c["t"], len(c["t"]))
            stages.append(FC.expected_stage(ia, da, c["pos"], FC.RATIO, FC.CD, nn))
        for name, s in ((n, FC.EXPECT_STAGE_NN50[n]) for n in a["expect"].values()):
            qi = [k for k, v in a["expect"].items() if v == name][0]
            assert stages[0][qi] == stages[2][qi] == (s if nn == 50 else 0), name
        before = ctx.fginn32_group_counters()
        got = ctx.rep_match_group_f32(rq, parts, HES, typ, FC.RATIO, FC.CD, nn)
        d = _delta(ctx, before)
        want_open = sum(int((s >= 1).sum()) for s in stages)
        assert d["resolve_queries"] == want_open and d["resolve_launches"] == (1 if want_open else 0) and d["launch_sets"] == 1
        assert (want_open > 10) == (nn == 50)
        for g, c in zip(got, (a, mid, b)):
            FC.same_tents(g, oracle.match_fginn(a["q"], c["t"], c["pos"], FC.RATIO, FC.CD, nn))
        for r in parts + [rq]:
            r.free()


# ---- 5. growth -------------------------------------------------------------------------------------------------------------------
def test_appends_in_parts_across_the_first_capacity_and_failed_appends(modsx, oracle, ctx):
    with _Gpu():
        dim, n2 = 64, modsx.REP_F32_FIRST_ROWS + 1004
        c = FC.random_case(40, n2, dim, 77)
        regs = _regs_at(modsx, c["pos"])
        rq, typ = _slot(modsx, ctx, c["q"])
        whole, _ = _slot(modsx, ctx, c["t"], c["pos"])
        cuts = [0, 3000, 5000, n2]                                # the second append crosses the first capacity
        assert cuts[1] < modsx.REP_F32_FIRST_ROWS < cuts[2]
        parts = modsx.Rep(ctx)
        for a, b in zip(cuts, cuts[1:]):
            assert parts.append_f32(regs[a:b], c["t"][a:b], HES, typ) == b - a
            assert parts.count_f32(HES, typ) == b
        ref = oracle.match_fginn(c["q"], c["t"], c["pos"], FC.RATIO, FC.CD, 50)
        assert len(ref) > 10
        FC.same_tents(ctx.rep_match_fginn_f32(rq, whole, HES, typ, FC.RATIO, FC.CD, 50), ref)
        FC.same_tents(ctx.rep_match_fginn_f32(rq, parts, HES, typ, FC.RATIO, FC.CD, 50), ref)
        gr, gd = parts.class_f32(HES, typ)
        assert gd.dtype == np.float32 and np.array_equal(gd.view(np.uint32), c["t"].view(np.uint32)) and same_records(gr, regs)
        # failed appends: the class keeps its count, its rows and its matches
        more = c["t"][:5].copy()
        for bad_rows in (np.where(np.arange(5)[:, None] == 2, np.float32(np.nan), more), np.where(np.arange(5)[:, None] == 4, np.float32(2e17), more),
                         np.zeros((5, dim + 4), np.float32), np.zeros((5, 144), np.float32)):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+"):
                parts.append_f32(regs[:5], bad_rows, HES, typ)
            assert parts.count_f32(HES, typ) == n2
        gd2 = parts.class_f32(HES, typ)[1]
        assert np.array_equal(gd2.view(np.uint32), c["t"].view(np.uint32))
        FC.same_tents(ctx.rep_match_fginn_f32(rq, parts, HES, typ, FC.RATIO, FC.CD, 50), ref)
        # ... and takes the next good append: the rows of the failed ones left nothing behind
        assert parts.append_f32(regs[:5], more, HES, typ) == 5
        t2, p2 = np.concatenate([c["t"], more]), np.concatenate([c["pos"], c["pos"][:5]])
        FC.same_tents(ctx.rep_match_fginn_f32(rq, parts, HES, typ, FC.RATIO, FC.CD, 50), oracle.match_fginn(c["q"], t2, p2, FC.RATIO, FC.CD, 50))
        for r in (rq, whole, parts):
            r.free()


# ---- 6. describe_append ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oriented(ctx, modsx, small_pair):
    """image a of the small pair in HBM and its oriented, reprojected regions"""
    a = small_pair[0]
    im = ctx.upload(a)
    k = ctx.detect_affine_keypoints(im, modsx.default_hessaff_params())
    ro = ctx.detect_orientation(im, modsx.detect_affine_regions(k))
    regs = modsx.reproject_regions(ro, np.eye(3), a.shape[1], a.shape[0])
    assert len(regs) > 69
    yield a, im, regs
    im.free()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


DAISY_PAR = (15, 3, 8, 8, 0)


@pytest.mark.parametrize("typ", [SURF, LIOP, DAISY])
def test_describe_append_rows_equal_describe_regions(ctx, modsx, oriented, typ):
    with _Gpu():
        _, im, regs = oriented
        kw = dict(daisy_par=DAISY_PAR) if typ == DAISY else {}
        single = {SURF: ctx.describe_regions_surf, LIOP: ctx.describe_regions_liop,
                  DAISY: lambda i, r: ctx.describe_regions_daisy(i, r, rad=15, radq=3, thq=8, histq=8, nrm_type=0)}[typ]
        sift_before = ctx.describe_regions(im, regs[:69])
        want = single(im, regs[:69])
        assert want.shape[1] == {SURF: 64, LIOP: 144, DAISY: 200}[typ] and np.isfinite(want).all()
        rep = modsx.Rep(ctx)
        at = 0
        for n in (0, 1, 3, 65):                                   # the appends stack: rows 0, 1..3, 4..68
            assert rep.describe_append(im, regs[at:at + n], HES, typ, **kw) == n
            at += n
            gr, gd = rep.class_f32(HES, typ)
            assert len(gd) == at and same_records(gr, regs[:at])
            assert np.array_equal(_bits(gd), _bits(want[:at])) if at else gd.shape == (0, 0)      # an empty class has no width yet
        fresh = modsx.Rep(ctx)
        assert fresh.describe_append(im, regs[:65], MSER, typ, **kw) == 65
        assert np.array_equal(_bits(fresh.class_f32(MSER, typ)[1]), _bits(want[:65]))
        assert fresh.count_f32(HES, typ) == 0
        # matching the class against itself: what the single-problem entry gives for these rows
        pos = np.stack([regs["reproj_kp"]["x"][:69], regs["reproj_kp"]["y"][:69]], 1)
        FC.same_tents(ctx.rep_match_fginn_f32(rep, rep, HES, typ), ctx.match_fginn_f32(want, want, pos))
        assert np.array_equal(_bits(ctx.describe_regions(im, regs[:69])), _bits(sift_before))
        rep.free(); fresh.free()


def test_describe_append_refuses_a_surf_list_with_nan_rows(ctx, modsx, oriented):
    with _Gpu():
        _, im, regs = oriented
        rep = modsx.Rep(ctx)
        assert rep.describe_append(im, regs[:7], HES, SURF) == 7
        before = rep.class_f32(HES, SURF)[1]
        assert np.isnan(ctx.describe_regions_surf(im, regs[7:12], mr_size=100.0)).all()      # Haar size 0: the reference's NaN rows
        with pytest.raises(RuntimeError, match=r"\(-1\): .+finite"):
            rep.describe_append(im, regs[7:12], HES, SURF, mr_size=100.0)
        assert rep.count_f32(HES, SURF) == 7 and np.array_equal(_bits(rep.class_f32(HES, SURF)[1]), _bits(before))
        assert rep.describe_append(im, regs[7:12], HES, SURF) == 5
        assert np.array_equal(_bits(rep.class_f32(HES, SURF)[1]), _bits(ctx.describe_regions_surf(im, regs[:12])))
        rep.free()


def test_a_refused_first_append_leaves_an_empty_class_that_takes_any_width_next(ctx, modsx, oracle, oriented):
    """A first append that the pack kernel's flag refuses must not leave the class a buffer sized for that call's kernel width: the
    class is still empty and has no width, so the next append may be of any width its type has.  DAISY is the type whose kernel
    width varies (32 .. 256); its kernel saturates the patch to bytes, so no pixel value gives it an invalid row, and the refusal
    is produced with SURF's NaN rows (kernel width 64) while the wide rows go into DAISY and CAFFE classes of the same
    representation, each refused or empty first."""
    with _Gpu():
        _, im, regs = oriented
        rep = modsx.Rep(ctx)
        with pytest.raises(RuntimeError, match=r"\(-1\): .+finite"):
            rep.describe_append(im, regs[:40], HES, SURF, mr_size=100.0)
        assert rep.count_f32(HES, SURF) == 0 and rep.class_f32(HES, SURF)[1].shape == (0, 0)
        # the refused class takes rows afterwards and matches like the single-problem entry
        assert rep.describe_append(im, regs[:40], HES, SURF) == 40
        want = ctx.describe_regions_surf(im, regs[:40])
        assert np.array_equal(_bits(rep.class_f32(HES, SURF)[1]), _bits(want))
        pos = np.stack([regs["reproj_kp"]["x"][:40], regs["reproj_kp"]["y"][:40]], 1)
        FC.same_tents(ctx.rep_match_fginn_f32(rep, rep, HES, SURF), oracle.match_fginn(want, want, pos, 0.8, 30.0, 50))
        # a narrow DAISY append (dim 32, kernel width 32) on an image of NaN pixels is NOT refused: the rows are finite
        nan_im = ctx.upload(np.full((240, 320), np.nan, np.float32))
        narrow = modsx.Rep(ctx)
        assert narrow.describe_append(nan_im, regs[:600], HES, DAISY, daisy_par=(15, 1, 3, 8, 0)) == min(600, len(regs))
        assert np.isfinite(narrow.class_f32(HES, DAISY)[1]).all() and narrow.class_f32(HES, DAISY)[1].shape[1] == 32
        nan_im.free()
        # ... so the widths stay apart by the class's own rule: a wide append to that class is refused, a fresh class takes it
        wide = ctx.describe_regions_daisy(im, regs[:69], rad=15, radq=3, thq=8, histq=8, nrm_type=0)
        with pytest.raises(RuntimeError, match=r"\(-1\): .+another width"):
            narrow.append_f32(regs[:69], wide, HES, DAISY)
        fresh = modsx.Rep(ctx)
        assert fresh.append_f32(regs[:69], wide, HES, DAISY) == 69
        pos = np.stack([regs["reproj_kp"]["x"][:69], regs["reproj_kp"]["y"][:69]], 1)
        FC.same_tents(ctx.rep_match_fginn_f32(fresh, fresh, HES, DAISY), oracle.match_fginn(wide, wide, pos, 0.8, 30.0, 50))
        for r in (rep, narrow, fresh):
            r.free()


def test_describe_append_in_sub_batches_of_four_in_a_child(ctx, modsx, oriented, tmp_path):
    with _Gpu():
        assert not os.environ.get("MODSX_LIOP_BATCH"), "this module is about the default sub-batch in the parent"
        a, im, regs = oriented
        inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
        np.savez(inp, image=a, regs=np.frombuffer(np.ascontiguousarray(regs[:9], modsx.REGION).tobytes(), np.uint8), mr_size=5.1962)
        p = subprocess.run([sys.executable, CHILD, inp, outp], env=dict(os.environ, MODSX_LIOP_BATCH="4"), timeout=CHILD_TIMEOUT_S,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = p.stderr.decode(errors="replace")[-1500:]
        if p.returncode < 0 or p.returncode in (134, 139):
            pytest.exit("the describe_append child ended with status %d; nothing more is started on the GPU.  Its stderr ended:\n%s"
                        % (p.returncode, err), returncode=1)
        assert p.returncode == 0, "the describe_append child failed with status %d:\n%s" % (p.returncode, err)
        z = np.load(outp)
        assert int(z["batch"]) == 4 and int(z["n"]) == 9
        assert np.array_equal(_bits(z["rows"]), _bits(ctx.describe_regions_liop(im, regs[:9])))
        cnt = dict(zip(modsx.LIOP_COUNTERS, (int(v) for v in z["counters"])))
        assert (cnt["calls"], cnt["regions"], cnt["sub_batches"]) == (1, 9, 3), cnt        # 4 + 4 + 1: two cuts


# ---- 7. match_reps -----------------------------------------------------------------------------------------------------------------
def _planted_pair(modsx, n=600, dim=144, seed=5, matched=400):
    """n regions per side: `matched` of the second side are the first side's under a homography (row + noise), the rest is clutter"""
    rs = np.random.RandomState(seed)
    H = np.array([[1.1, 0.05, 20], [-0.03, 0.95, -10], [1e-5, 2e-5, 1]])
    p1 = rs.uniform(20, 900, (n, 2))
    x = np.c_[p1, np.ones(n)] @ H.T
    p2 = x[:, :2] / x[:, 2:] + rs.normal(0, 0.5, (n, 2))
    d1 = rs.randn(n, dim).astype(np.float32)
    d2 = (d1 + 0.25 * rs.randn(n, dim)).astype(np.float32)
    d2[matched:] = rs.randn(n - matched, dim)
    p2[matched:] = rs.uniform(20, 900, (n - matched, 2))
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


def _same_pair_result(got, ref):
    for k in ("n_regions", "n_tentatives", "n_unique", "n_ransac_inliers", "n_verified", "ransac_samples", "ransac_lo"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    FC.same_tents(got["tentatives"], ref["tentatives"])
    assert np.array_equal(got["ransac_inlier"], ref["ransac_inlier"]) and np.array_equal(got["verified"], ref["verified"])
    assert got["H"].tobytes() == ref["H"].tobytes()


def _params(modsx, use_f, seed=1):
    return modsx.default_pair_params(ransac_seed=seed, useF=1, LAFCoef=2.0, err_threshold=4.0) if use_f else \
        modsx.default_pair_params(ransac_seed=seed)


@pytest.mark.parametrize("use_f", [0, 1])
def test_match_reps_with_one_float_class_equals_match_regions_f32(ctx, modsx, use_f):
    with _Gpu():
        r1, d1, r2, d2 = _planted_pair(modsx)
        par = _params(modsx, use_f)
        ref = ctx.match_regions_f32(r1, d1, r2, d2, par)
        assert ref["n_verified"] >= 200
        ra, rb = modsx.Rep(ctx), modsx.Rep(ctx)
        ra.append_f32(r1, d1, HES, LIOP); rb.append_f32(r2, d2, HES, LIOP)
        _same_pair_result(modsx.match_reps([ctx], ra, [rb], par, [(HES, LIOP, par.match_ratio)])[0], ref)
        _same_pair_result(modsx.match_reps([ctx], ra, [rb], par)[0], ref)       # n_classes == 0: every non-empty class
        ra.free(); rb.free()


def _float_rows_of(desc_u8, dim):
    """deterministic float rows that keep the neighbourhoods of the u8 descriptors: no integers, another scale per width"""
    d = desc_u8.astype(np.float32)
    return np.ascontiguousarray(np.concatenate([d, d[:, :16]], 1) * np.float32(0.37) if dim == 144 else d[:, 32:96] * np.float32(1.3) + np.float32(0.5))


def _tail(lib, l1, l2, tent, par, seed):
    pts = np.stack([l1["reproj_kp"]["x"][tent["q"]], l1["reproj_kp"]["y"][tent["q"]],
                    l2["reproj_kp"]["x"][tent["t0"]], l2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = lib.duplicate_filtering(pts, tent["ratio"], par.duplicateDist, True)
    sel = order[keep]
    tu, pu = tent[sel], pts[sel]
    rr = lib.loransac_h(pu, laf_of(l1, tu["q"]), laf_of(l2, tu["t0"]), err_threshold=par.err_threshold, confidence=par.confidence,
                        max_samples=par.max_samples, lo=par.localOptimization, hlaf_coef=par.HLAFCoef, sym_check=par.doSymmCheck,
                        seed=seed, error_type=par.errorType)
    return tu, rr


@pytest.fixture(scope="module")
def mixed(ctx, modsx, small_pair):
    """RootSIFT + LIOP + SURF on the region lists of a HessianAffine and an MSER step of the small pair: (ra, rb, classes)"""
    a, b, _ = small_pair
    par = modsx.default_pair_params(ransac_seed=6)
    steps = [(modsx.set_vs_pars([1.0], [1], 360.0, 0.2, 1, []), HES), (modsx.set_vs_pars([1.0], [1], 360.0, 0.8, 1, []), MSER)]
    reps = []
    for g in (a, b):
        im = ctx.upload(g)
        rep = modsx.Rep(ctx)
        for views, det in steps:
            assert rep.add_views(im, views, par, detector=det) > 20
            regs, d = rep.regions(det, 1)
            rep.append_f32(regs, _float_rows_of(d, 144), det, LIOP)
            rep.append_f32(regs, _float_rows_of(d, 64), det, SURF)
        im.free()
        reps.append(rep)
    classes = [(det, typ) for typ in (1, LIOP, SURF) for det in (HES, MSER)]
    yield reps[0], reps[1], classes
    for r in reps:
        r.free()


def _class_lists(modsx, ctx, ra, rb, classes, par):
    """the per-class region lists and tentatives (from the per-class taps) in the order of rep_class_rank, re-based"""
    l1, l2, tents = [], [], []
    for det, typ in sorted(classes, key=lambda k: modsx.rep_class_rank(*k)):
        if typ < 8:
            g1, g2 = ra.regions(det, typ, want_desc=False), rb.regions(det, typ, want_desc=False)
            t = ctx.rep_match_fginn(ra, rb, det, typ, par.match_ratio, par.contradDist, par.nn)
        else:
            g1, g2 = ra.class_f32(det, typ)[0], rb.class_f32(det, typ)[0]
            t = ctx.rep_match_fginn_f32(ra, rb, det, typ, par.match_ratio, par.contradDist, par.nn)
        t = t.copy()
        t["q"] += sum(len(x) for x in l1)
        for f in ("t0", "tj", "t1"):
            t[f] = np.where(t[f] >= 0, t[f] + sum(len(x) for x in l2), t[f])
        l1.append(g1); l2.append(g2); tents.append(t)
    return np.concatenate(l1), np.concatenate(l2), tents


def test_match_reps_mixed_classes_concatenate_in_rank_order(ctx, modsx, oracle, mixed):
    need_ref(oracle)
    with _Gpu():
        ra, rb, classes = mixed
        par = modsx.default_pair_params(ransac_seed=6)
        ranks = [modsx.rep_class_rank(*k) for k in classes]
        assert sorted(ranks) != ranks                             # the call lists them in another order than they are concatenated in
        got = modsx.match_reps([ctx], ra, [rb], par, [(d, t, par.match_ratio) for d, t in classes])[0]
        l1, l2, tents = _class_lists(modsx, ctx, ra, rb, classes, par)
        assert all(len(t) > 5 for t in tents)
        tent = np.concatenate(tents)
        assert got["n_regions"] == (len(l1), len(l2)) and got["n_tentatives"] == len(tent)
        # the float tentatives are the single-problem entry's on the class's rows
        rows1, rows2 = ra.class_f32(HES, LIOP)[1], rb.class_f32(HES, LIOP)[1]
        g2 = rb.class_f32(HES, LIOP)[0]
        pos2 = np.stack([g2["reproj_kp"]["x"], g2["reproj_kp"]["y"]], 1)
        FC.same_tents(ctx.rep_match_fginn_f32(ra, rb, HES, LIOP, par.match_ratio, par.contradDist, par.nn),
                      oracle.match_fginn(rows1, rows2, pos2, par.match_ratio, par.contradDist, par.nn))
        for lib in (modsx, oracle):
            tu, rr = _tail(lib, l1, l2, tent, par, 6)
            assert got["n_unique"] == len(tu)
            FC.same_tents(got["tentatives"], tu)
            assert np.array_equal(got["ransac_inlier"], rr["inl"]) and np.array_equal(got["verified"], rr["keep"])
            assert got["n_verified"] == rr["n"] > 20
            assert np.abs(normH(got["H"]) - normH(rr["H"])).max() < 1e-4
        # n_classes == 0 takes every non-empty class: the same six
        _same_pair_result(modsx.match_reps([ctx], ra, [rb], par)[0], got)


def test_match_reps_nine_partners_over_two_contexts(ctx, modsx):
    with _Gpu():
        other = modsx.Context(0)
        par = _params(modsx, 0)
        r1, d1, _, _ = _planted_pair(modsx, 300, 64, 5, 200)
        ra = modsx.Rep(ctx)
        ra.append_f32(r1, d1, SURFDET, SURF)
        reps, refs = [], []
        for i in range(9):
            n = (0, 3, 120, 300)[i % 4] if i < 8 else 300
            _, _, r2, d2 = _planted_pair(modsx, 300, 64, 5 + i // 4, 200)      # seed 5: the partner of r1; the others are unrelated
            rb = modsx.Rep(ctx)
            rb.append_f32(r2[:n], d2[:n], SURFDET, SURF, ctx=(ctx, other)[i % 2])
            reps.append(rb)
            refs.append(ctx.match_regions_f32(r1, d1, r2[:n], d2[:n], par))
        before = ctx.fginn32_group_counters()["launch_sets"] + other.fginn32_group_counters()["launch_sets"]
        got = modsx.match_reps([ctx, other], ra, reps, par)
        sets = ctx.fginn32_group_counters()["launch_sets"] + other.fginn32_group_counters()["launch_sets"] - before
        assert 3 <= sets <= 5                                     # groups of up to four partners, not nine single problems
        for g, ref in zip(got, refs):
            _same_pair_result(g, ref)
        assert got[3]["n_verified"] > 50 and got[0]["n_regions"] == (300, 0) and (got[0]["H"] == -1).all()
        for r in reps + [ra]:
            r.free()
        other.close()


def test_match_reps_database_changes_the_rootsift_class_only(ctx, modsx, mixed):
    with _Gpu():
        ra, rb, classes = mixed
        par = modsx.default_pair_params(ransac_seed=6)
        n_float = sum(ra.count_f32(d, t) for d, t in classes if t >= 8)
        plain = modsx.match_reps([ctx], ra, [rb], par)[0]
        rs = np.random.RandomState(11)
        qd = np.concatenate([ra.regions(HES, 1)[1], ra.regions(MSER, 1)[1]]).astype(np.int64)
        near = np.clip(qd[::2] + rs.randint(-3, 4, qd[::2].shape), 0, 255)
        rows = np.concatenate([near, rs.randint(0, 60, (4096 - len(near), 128))]).astype(np.uint8)
        db = ctx.db_create(rows)
        ctx.set_fginn_db(db)
        try:
            got = modsx.match_reps([ctx], ra, [rb], par)[0]
            taps = [ctx.rep_match_fginn_f32(ra, rb, d, t, par.match_ratio, par.contradDist, par.nn) for d, t in classes if t >= 8]
        finally:
            ctx.set_fginn_db(None)
        db.free()
        # the float classes give what they gave without the database; only the RootSIFT classes lose tentatives
        plain_taps = [ctx.rep_match_fginn_f32(ra, rb, d, t, par.match_ratio, par.contradDist, par.nn) for d, t in classes if t >= 8]
        for x, y in zip(taps, plain_taps):
            FC.same_tents(x, y)
        n_float_tents = sum(len(t) for t in taps)
        assert n_float > 0 and n_float_tents > 20
        assert 0 < got["n_tentatives"] - n_float_tents < plain["n_tentatives"] - n_float_tents


# ---- 8. key-file round trip --------------------------------------------------------------------------------------------------------
def test_key_file_round_trip_into_a_float_class(modsx, oracle, ctx, tmp_path):
    with _Gpu():
        rs = np.random.RandomState(77)
        t = rs.randint(-999, 1000, (130, 144)).astype(np.float32) / 8      # eighths: exact in the key file's six digits
        q = t[rs.randint(0, 130, 65)] + rs.randint(-40, 41, (65, 144)).astype(np.float32) / 8
        pos = np.round(rs.uniform(0, 100, (130, 2)) * 8) / 8
        path = os.path.join(str(tmp_path), "liop.txt")
        reps = []
        for rows, p in ((q, np.zeros((65, 2))), (t, pos)):
            r = _regs_at(modsx, p)
            r["det_kp"]["x"], r["det_kp"]["y"] = p[:, 0], p[:, 1]
            r["reproj_kp"]["a11"] = r["reproj_kp"]["a22"] = r["det_kp"]["a11"] = r["det_kp"]["a22"] = 1
            r["reproj_kp"]["s"] = r["det_kp"]["s"] = 3
            modsx.save_regions(path, [("HessianAffine", "LIOP", r, rows, 144)])
            _, dn, lr, ld = modsx.load_regions(path, "HessianAffine", "LIOP")
            assert dn == "LIOP" and np.array_equal(ld, rows) and np.array_equal(lr["reproj_kp"]["x"], p[:, 0])
            rep = modsx.Rep(ctx)
            assert rep.append_f32(lr, ld, HES, LIOP) == len(rows)
            reps.append(rep)
        ref = oracle.match_fginn(q, t, pos, FC.RATIO, FC.CD, 50)
        assert 10 < len(ref) <= len(q)
        FC.same_tents(ctx.rep_match_fginn_f32(reps[0], reps[1], HES, LIOP), ref)
        FC.same_tents(ctx.match_fginn_f32(q, t, pos), ref)
        for r in reps:
            r.free()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_context_and_representation_usable(ctx, modsx, oracle, oriented):
    with _Gpu():
        _, im, oregs = oriented
        c = FC.random_case(65, 130, 64, 3)
        rq, rt = modsx.Rep(ctx), modsx.Rep(ctx)
        regs_q, regs_t = _regs_at(modsx, np.zeros((65, 2))), _regs_at(modsx, c["pos"])
        rq.append_f32(regs_q, c["q"], HES, SURF); rt.append_f32(regs_t, c["t"], HES, SURF)
        ok = oracle.match_fginn(c["q"], c["t"], c["pos"], FC.RATIO, FC.CD, 50)

        def refused(fn, what=r".+"):
            with pytest.raises(RuntimeError, match=r"\(-1\): " + what):      # MODSX_ERR_ARG with a message
                fn()
            assert rq.count_f32(HES, SURF) == 65 and rt.count_f32(HES, SURF) == 130
            FC.same_tents(ctx.rep_match_fginn_f32(rq, rt, HES, SURF), ok)

        for det in (1, 2, 4, 7):                                  # DoG, Harris, numbers that name no detector
            refused(lambda: rt.append_f32(regs_t, c["t"], det, SURF))
            refused(lambda: rt.class_f32(det, SURF))
            refused(lambda: ctx.rep_match_fginn_f32(rq, rt, det, SURF))
            refused(lambda: rt.describe_append(im, oregs[:3], det, SURF))
        for typ in (0, 1, 3, 4, 7, 13):
            refused(lambda: rt.append_f32(regs_t, c["t"], HES, typ))
            refused(lambda: ctx.rep_match_group_f32(rq, [rt], HES, typ))
            refused(lambda: modsx.match_reps([ctx], rq, [rt], modsx.default_pair_params(), [(HES, typ, 0.8)]) if typ > 3 else rt.class_f32(HES, typ))
        # widths: what the type does not have, what the class does not hold, what the matcher does not take
        for typ, dim in ((SURF, 128), (LIOP, 64), (MROGH, 144), (DAISY, 20), (DAISY, 144), (CAFFE, 6), (CAFFE, 260), (CAFFE, 0)):
            refused(lambda: rt.append_f32(regs_t[:4], np.zeros((4, dim), np.float32), HES, typ), r".*width")
        caffe = modsx.Rep(ctx)
        assert caffe.append_f32(regs_t[:4], np.zeros((4, 128), np.float32), HES, CAFFE) == 4
        refused(lambda: caffe.append_f32(regs_t[:4], np.zeros((4, 64), np.float32), HES, CAFFE), r".*another width")
        wide = modsx.Rep(ctx)
        wide.append_f32(regs_t[:4], np.zeros((4, 64), np.float32), HES, CAFFE)
        refused(lambda: ctx.rep_match_fginn_f32(caffe, wide, HES, CAFFE), r".*widths")
        for bad in (np.nan, np.inf, -np.inf, 1.1e17, -2e17):
            rows = c["t"][:6].copy()
            rows[3, 9] = bad
            refused(lambda: rt.append_f32(regs_t[:6], rows, HES, SURF), r".*finite")
        # describe_append: no extractor for CAFFE / MROGH, the extractor's own rules
        for typ in (CAFFE, MROGH):
            refused(lambda: rt.describe_append(im, oregs[:3], HES, typ), r".*extractor")
        refused(lambda: rt.describe_append(im, oregs[:3], HES, DAISY), r".*daisy_par")
        refused(lambda: rt.describe_append(im, oregs[:3], HES, DAISY, daisy_par=(15, 4, 8, 8, 0)))
        refused(lambda: rt.describe_append(im, oregs[:3], HES, SURF, patch_size=31), r".*41")
        refused(lambda: rt.describe_append(im, oregs[:3], HES, LIOP, patch_size=31), r".*41")
        refused(lambda: rt.describe_append(im, oregs[:3], HES, SURF, mr_size=0.0), r".*mrSize")
        # the matcher's limits
        for nn in (1, 257):
            refused(lambda: ctx.rep_match_fginn_f32(rq, rt, HES, SURF, nn=nn))
        for ratio in (float("nan"), 1.0, -1.5):
            refused(lambda: ctx.rep_match_group_f32(rq, [rt, rt], HES, SURF, ratio=ratio))
        refused(lambda: ctx.rep_match_group_f32(rq, [], HES, SURF))
        refused(lambda: ctx.rep_match_group_f32(rq, [rt] * 5, HES, SURF))
        # more than 2 000 000 regions in a class: refused before anything is read
        L = modsx.lib()
        assert L.modsx_rep_append_f32(ctx.h, rt.h, HES, SURF, regs_t.ctypes.data, c["t"].ctypes.data, 64, 2000001 - 130) == -1
        assert rt.count_f32(HES, SURF) == 130
        # the u8 entries keep refusing the float types
        refused(lambda: rt.append(regs_t[:4], np.zeros((4, 128), np.uint8), HES, SURF))
        refused(lambda: ctx.rep_match_fginn(rq, rt, HES, LIOP))
        for r in (rq, rt, caffe, wide):
            r.free()
