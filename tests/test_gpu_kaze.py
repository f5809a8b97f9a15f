"""GPU: the KAZE detector, bit for bit against tests/kaze_model.py -- the restatement of AKAZE's nonlinear scale space and
Hessian extrema that tests/test_kaze_model_cpu.py ties to the compiled reference -- on the images, parameter sets and planted
planes of tests/kaze_cases.py: every plane and list of the debug tap, sizes on each side of every tile size, the scan entry on the
planted planes against the fixture, the keypoints and their order, a batch of mixed sizes against single calls, the counters, the
flat image, the chain detect_kaze -> kaze_regions -> detect_affine_shape -> detect_orientation -> describe_regions -> match_fginn,
and a describe call around a KAZE call.  Planes compare with -0 equal to +0 and NaN equal to NaN (nothing downstream tells them
apart); lists and keypoints compare as bits."""
import os

import numpy as np
import pytest

import kaze_cases as KC
import kaze_model as M
from surfdet_cases import blobs

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kaze_ref.npz")
LISTS = ("raw", "rawv", "aux", "upper", "final")


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


def params(modsx, par):
    return modsx.kaze_params(**par)


def same_lists(got, want, what):
    for key in LISTS:
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, key)


def same_keypoints(modsx, got, final, what=""):
    want = M.keypoints(final, modsx.KEYPOINT)
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    for f in got.dtype.names:                             # every field as bits, the -0.0 of a21 included
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


def same_tap(tap, m, what):
    assert len(tap["Lt"]) == len(m["levels"]), what
    assert tap["kcontrast"] == m["kcontrast"] or (np.isnan(tap["kcontrast"]) and np.isnan(m["kcontrast"])), (what, tap["kcontrast"], m["kcontrast"])
    assert tap["hmax"] == m["hmax"], (what, tap["hmax"], m["hmax"])
    assert np.array_equal(tap["hist"], m["hist"]), what
    for name in ("Lt", "Lsmooth", "Lflow", "Ldet"):
        for i, (g, w) in enumerate(zip(tap[name], m[name])):
            if not M.same(g, w):
                bad = np.nonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))
                raise AssertionError("%s: %s of level %d: %d of %d values differ, first at (%d, %d): %r != %r" %
                                     (what, name, i, len(bad[0]), g.size, bad[0][0], bad[1][0], g[bad[0][0], bad[1][0]], w[bad[0][0], bad[1][0]]))
    same_lists(tap, m, what)


@pytest.mark.parametrize("name", KC.names())
def test_every_plane_every_list_and_the_keypoints(ctx, modsx, fixture, name):
    _, img, par = KC.case(name)
    m = KC.model(name)
    im = ctx.upload(img)
    try:
        tap = ctx.debug_kaze(im, params(modsx, par))
        kps = ctx.detect_kaze(im, params(modsx, par))
    finally:
        im.free()
    same_tap(tap, m, name)
    same_keypoints(modsx, kps, m["final"], name)
    # ... and the fixture's keypoints, in value and order
    k = list(fixture["names"]).index(name)
    same_keypoints(modsx, kps, fixture["c%02d_final" % k], name + " (fixture)")


def _tile_sizes(modsx):
    t = modsx.kaze_geometry(96, 128)["tiles"]
    w, h = t["width"], t["height"]
    # one width and one row count on each side of a stencil tile (and of the 64 x 4 tiles of the diffusion step), and a width that
    # is a multiple of 4 with a partial last tile: the 16-byte loads and the scalar loads in one row of tiles
    return [(w - 1, 50), (w + 1, 50), (70, h - 1), (70, h + 1), (w + 4, 2 * h + 1), (2 * w, 3), (3, 40)]


@pytest.mark.parametrize("k", range(7))
def test_sizes_on_each_side_of_the_tile_sizes(ctx, modsx, k):
    w, h = _tile_sizes(modsx)[k]
    img = blobs(w, h, seed=3)
    m = M.detect(img)
    im = ctx.upload(img)
    try:
        tap = ctx.debug_kaze(im)
    finally:
        im.free()
    same_tap(tap, m, "%d x %d" % (w, h))


@pytest.mark.parametrize("name", sorted(KC.PLANTED))
def test_scan_on_the_planted_planes(ctx, modsx, fixture, name):
    (w, h), par, _ = KC.PLANTED[name]
    _, _, planes = KC.planted(name)
    got = ctx.debug_kaze_scan(h, w, planes, params(modsx, par))
    want = {key: fixture["p_%s_%s" % (name, key)] for key in LISTS}
    assert len(want["raw"]) > 0 and len(want["final"]) > 0
    same_lists(got, want, name)


def test_batch_of_mixed_sizes_equals_single_calls_and_the_counters(ctx, modsx):
    cases = [KC.case(n) for n in KC.BATCH]
    assert len({c[1].shape for c in cases}) == len(cases)
    want = [KC.model(n)["final"] for n in KC.BATCH]
    assert sum(len(w) for w in want) > 0
    par = modsx.kaze_params()
    ims = [ctx.upload(img) for _, img, _ in cases]
    try:
        before = ctx.kaze_counters()
        got = ctx.detect_kaze_batch(ims, par)
        d = {k: v - before[k] for k, v in ctx.kaze_counters().items()}
        singles = [ctx.detect_kaze(im, par) for im in ims]
        back = ctx.detect_kaze_batch(ims[::-1], par)[::-1]
        assert ctx.detect_kaze_batch([], par) == []
    finally:
        for im in ims:
            im.free()
    for g, s, b, w, name in zip(got, singles, back, want, KC.BATCH):
        same_keypoints(modsx, g, w, "batch, " + name)
        same_keypoints(modsx, s, w, "single, " + name)
        same_keypoints(modsx, b, w, "reversed batch, " + name)
    models = [KC.model(n) for n in KC.BATCH]
    # one launch per diffusion step over the whole batch: the steps of the image with the most levels
    steps = max((sum(len(L["tau"]) for L in m["levels"]) for m in models))
    assert d["calls"] == 1 and d["images"] == len(cases) and d["fed_steps"] == steps, d
    assert d["raw_maxima"] == sum(len(m["raw"]) for m in models) and d["survivors"] == sum(len(m["upper"]) for m in models), d
    assert d["keypoints"] == sum(len(w) for w in want), d
    # the histograms, the count of maxima, the maxima, the nine values: one wait each per batch
    assert d["host_waits"] == 4, d


def test_flat_image_gives_no_keypoint_and_no_error(ctx, modsx):
    _, img, par = KC.case("flat_128x96")
    im = ctx.upload(img)
    try:
        assert len(ctx.detect_kaze(im, params(modsx, par))) == 0
        tap = ctx.debug_kaze(im, params(modsx, par))
    finally:
        im.free()
    assert tap["kcontrast"] == 0 and tap["hmax"] == 0 and len(tap["raw"]) == 0
    # k = 0: the conductivity is 0 * inf everywhere, so every diffused pixel is NaN; the corners, which no step writes, stay finite
    assert np.isnan(tap["Lflow"][1]).all() and np.isnan(tap["Lt"][1][1:-1]).all() and np.isfinite(tap["Lt"][1][0, 0])
    assert np.isnan(tap["Ldet"][2]).any()


def _f32_scales_with_the_same_ratio(AM, s):
    """tests/affshape_model.py runs the oracle's Baumberg loop, which forms the ratio from an f32 scale.  A KAZE scale is size / 3.0,
    a double; its ratio (float)(s / (double)1.6f) is what the loop reads.  -> (s32, ok): an f32 scale with that same ratio, where one
    exists (four in five: the quotient's step is 1.25 ulp where 1.6 * ratio crosses into the next binade)"""
    ratio, _ = AM.ratio_res(s)
    c = np.float64(AM.SIGMA)
    mid = (ratio.astype(np.float64) * c).astype(np.float32)
    s32, ok = mid.copy(), np.zeros(len(s), bool)
    for cand in (mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))):
        hit = ~ok & ((cand.astype(np.float64) / c).astype(np.float32) == ratio)
        s32[hit], ok = cand[hit], ok | hit
    return s32, ok


def test_chain_on_the_small_pair(ctx, modsx, oracle, small_pair):
    """detect_kaze -> kaze_regions -> detect_affine_shape -> detect_orientation -> (identity reprojection) -> describe_regions ->
    match_fginn on the small synthetic pair: the reference's KAZE branch with doBaumberg = 1, against the same
    chain fed with the keypoints of tests/kaze_model.py and run by the oracle.  Step 3 goes through tests/affshape_model.py for
    every region whose ratio an f32 scale reproduces (the model's oracle path takes f32 scales only), and its border test for all."""
    from tests import affshape_model as AM
    from tests.common import same_records
    sides = []
    for k, g in enumerate(small_pair[:2]):
        final = M.detect(g)["final"]
        want = np.zeros(len(final), modsx.REGION)
        want["det_kp"] = M.keypoints(final, modsx.KEYPOINT)
        want["type"], want["id"], want["img_id"] = M.DET_KAZE, np.arange(len(final)), k
        im = ctx.upload(g)
        try:
            regs = modsx.kaze_regions(ctx.detect_kaze(im), img_id=k)
            adapted = ctx.detect_affine_shape(im, regs)
            ro = modsx.reproject_regions(ctx.detect_orientation(im, adapted), np.eye(3), g.shape[1], g.shape[0])
            desc = ctx.describe_regions(im, ro)
        finally:
            im.free()
        assert len(regs) == len(want) > 50 and same_records(regs, want), "KAZE regions of image %d" % k
        # step 3: no region the border test refuses comes back, and the shapes are the model's wherever the model can run
        border, _, _ = AM.border_test(oracle, want, g.shape[0], g.shape[1])
        assert 0.3 * len(want) < len(adapted) <= len(want) and not border[adapted["id"]].any()
        s32, ok = _f32_scales_with_the_same_ratio(AM, want["det_kp"]["s"])
        assert ok.mean() > 0.6
        sub = want[ok].copy()
        sub["det_kp"]["s"] = s32[ok].astype(np.float64)
        want_a, _ = AM.run(oracle, g, sub)
        want_a["det_kp"]["s"] = want["det_kp"]["s"][want_a["id"]]
        got_a = adapted[ok[adapted["id"]]]
        assert len(got_a) == len(want_a) and same_records(got_a, want_a), "adapted KAZE regions of image %d" % k
        # steps 4 to 6 by the oracle
        want_r = oracle.reproject_regions(oracle.detect_orientation(g, adapted), np.eye(3), g.shape[1], g.shape[0])
        want_d = oracle.describe_regions(g, want_r)
        assert len(ro) == len(want_r) > 20 and same_records(ro, want_r)
        assert desc.tobytes() == want_d.tobytes()
        sides.append((ro, desc, want_r, want_d))
    (r1, d1, w1, m1), (r2, d2, w2, m2) = sides
    pos2 = np.stack([w2["reproj_kp"]["x"], w2["reproj_kp"]["y"]], 1)
    tent = oracle.match_fginn(m1, m2, pos2, 0.8, 30.0, 50)
    got = ctx.match_fginn(d1, d2, np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1), 0.8, 30.0, 50)
    assert len(tent) > 0, "a chain without a tentative compares empty lists"
    assert same_records(got, tent)


def test_a_describe_call_is_unchanged_by_a_kaze_call(ctx, modsx, small_pair):
    a = small_pair[0]
    im = ctx.upload(a)
    try:
        regs = modsx.surf_regions(ctx.detect_surf(im))
        regs = modsx.reproject_regions(ctx.detect_orientation(im, regs), np.eye(3), a.shape[1], a.shape[0])
        before = ctx.describe_regions(im, regs)
        assert len(ctx.detect_kaze(im)) > 0
        after = ctx.describe_regions(im, regs)
    finally:
        im.free()
    assert len(before) > 0 and before.tobytes() == after.tobytes()
