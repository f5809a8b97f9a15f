"""GPU: external affine adaptation (DetectAffineShape, synth-detection.cpp:922-1074, on a caller's regions) against
tests/affshape_model.py -- the oracle's interpolateCheckBorders and findAffineShape behind the f64 ratio -- region by region.

Comparison rule, everywhere: bit equality.  Through Context.debug_affine_shape the border flag, the shape u[4], ok and iters of
EVERY input region equal the model's -- dropped regions included, with the state and the loop counter at the moment they left --
and no launched region is left unwritten (the entry fills the result buffer with 0xFF bytes: iters == -1 is reserved for
border-refused regions).  Through detect_affine_shape / detect_affine_shape_batch the region lists equal the model's field by
field.  No tolerance: same operands, same order, no contraction.

The cases are those of tests/affshape_cases.py; tests/test_affshape_cases_cpu.py proves without a device what they reach.
  1. the whole list at W = 19 through the production variant, the static stream kernel and both one-keypoint kernels
  2. every odd window 3..19 on a 40-region subset
  3. list prefixes around the two slots of a wavefront and the eight ranges of the queue
  4. maxIterations 1, 2, 16 and convergenceThreshold 0.01, 0.2
  5. the three images in one call against three single calls, with an empty list and an all-refused list among them
  6. one context shared with the scale-space detector (the queue counters' invariant)
  7. counters, the SURF chain, refusals
"""
import numpy as np
import pytest

from tests import affshape_cases as AC
from tests import affshape_model as AM
from tests.common import same_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dimgs(ctx, oracle):
    ims = [ctx.upload(p) for p in AC.images(oracle)]     # f32, 1 channel: stored unchanged
    yield ims
    for im in ims:
        im.free()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare_report(got, reps, what):
    """got: debug_affine_shape's dict over the concatenated lists; reps: the model's reports, one per image"""
    ref = {f: np.concatenate([r[f] for r in reps]) for f in ("border", "u", "ok", "iters", "reason")}
    n = len(ref["ok"])
    assert len(got["ok"]) == n, what
    assert np.array_equal(got["border"], ref["border"]), (what, "border test", np.nonzero(got["border"] != ref["border"])[0][:10])
    assert got["launched"] == int((~ref["border"]).sum()), what
    unwritten = np.nonzero((got["iters"] == -1) & ~ref["border"])[0]
    assert len(unwritten) == 0, (what, "regions no wavefront wrote", unwritten[:10])
    bad = np.nonzero((got["ok"] != ref["ok"]) | (got["iters"] != ref["iters"]) | (_bits(got["u"]) != _bits(ref["u"])).any(1))[0]
    if len(bad):
        k = int(bad[0])
        detail = dict(region=k, got=(got["u"][k].tolist(), int(got["ok"][k]), int(got["iters"][k])),
                      ref=(ref["u"][k].tolist(), int(ref["ok"][k]), int(ref["iters"][k]), int(ref["reason"][k])))
        raise AssertionError("%s: %d of %d regions differ from the model, first %r" % (what, len(bad), n, detail))


def _same_regions(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert same_records(got, want), what
    for f in ("a11", "a12", "a21", "a22"):          # as bits: the widened f32 shape
        assert got["det_kp"][f].tobytes() == want["det_kp"][f].tobytes(), (what, f)


def _run_debug(ctx, modsx, oracle, dimgs, which, regs, variant=-1, **params):
    """debug_affine_shape on the images `which` with the lists regs against the model"""
    got = ctx.debug_affine_shape([dimgs[i] for i in which], regs, modsx.default_affshape_params(**params), variant=variant)
    reps = [AM.run(oracle, AC.images(oracle)[i], r, **params)[1] for i, r in zip(which, regs)]
    _compare_report(got, reps, "images %r variant %d %r" % (which, variant, params))
    W = params.get("smmWindowSize", 19)
    v = modsx.baumberg_production_variant(W) if variant < 0 else variant
    assert got["geometry"] == ctx.baumberg_geometry(got["launched"], W, v, 0)
    return got


# ---------------------------------------------------------------------------------------------------------- 1. whole list
def test_whole_list_production_variant(ctx, modsx, oracle, dimgs):
    got = ctx.debug_affine_shape(dimgs, AC.regions())
    _compare_report(got, [rep for _, rep in AC.expected(oracle)], "production")
    assert modsx.baumberg_production_variant(19) == 3 and got["geometry"]["kernel"] == 3        # the queue form is what ships
    assert got["geometry"] == ctx.baumberg_geometry(got["launched"], 19, 3, 0)
    assert got["launched"] >= 300 and got["ok"].sum() >= 100


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_whole_list_every_kernel(ctx, modsx, oracle, dimgs, variant):
    got = ctx.debug_affine_shape(dimgs, AC.regions(), variant=variant)
    _compare_report(got, [rep for _, rep in AC.expected(oracle)], "variant %d" % variant)
    assert got["geometry"]["kernel"] == variant


def test_entries_give_the_models_lists(ctx, oracle, dimgs):
    for i, (im, regs) in enumerate(zip(dimgs, AC.regions())):
        _same_regions(ctx.detect_affine_shape(im, regs), AC.expected(oracle)[i][0], "image %d" % i)


# ------------------------------------------------------------------------------------------------------------- 2. windows
@pytest.mark.parametrize("W", [3, 5, 7, 9, 11, 13, 15, 17, 19])
def test_every_odd_window(ctx, modsx, oracle, dimgs, W):
    regs = AC.regions()[0][60:100]
    got = _run_debug(ctx, modsx, oracle, dimgs, [0], [regs], smmWindowSize=W)
    assert got["geometry"]["kernel"] == (3 if W == 19 else 2) and got["launched"] >= 20
    want, _ = AM.run(oracle, AC.images(oracle)[0], regs, smmWindowSize=W)
    _same_regions(ctx.detect_affine_shape(dimgs[0], regs, modsx.default_affshape_params(smmWindowSize=W)), want, "W %d" % W)
    _run_debug(ctx, modsx, oracle, dimgs, [0], [regs[:5]])          # and the default window again: the mask follows the window size


# ------------------------------------------------------------------------------------------------------------ 3. prefixes
@pytest.mark.parametrize("variant", [-1, 0])
def test_prefixes(ctx, modsx, oracle, dimgs, variant):
    regs = AC.regions()[0]
    launchable = np.nonzero(~AC.expected(oracle)[0][1]["border"])[0]
    for n in (1, 2, 3, 15, 16, 17, len(launchable)):
        # the shortest prefix of the list that launches n regions, and the n launched regions alone
        cut = regs[:launchable[n - 1] + 1]
        assert _run_debug(ctx, modsx, oracle, dimgs, [0], [cut], variant=variant)["launched"] == n
        assert _run_debug(ctx, modsx, oracle, dimgs, [0], [regs[launchable[:n]]], variant=variant)["launched"] == n


# ---------------------------------------------------------------------------------------------------------- 4. parameters
@pytest.mark.parametrize("iters", [1, 2, 16])
@pytest.mark.parametrize("th", [0.01, 0.2])
def test_iteration_caps_and_thresholds(ctx, modsx, oracle, dimgs, iters, th):
    regs = AC.regions()
    _run_debug(ctx, modsx, oracle, dimgs, [0, 1], regs[:2], maxIterations=iters, convergenceThreshold=th)
    par = modsx.default_affshape_params(maxIterations=iters, convergenceThreshold=th)
    want, _ = AM.run(oracle, AC.images(oracle)[0], regs[0], maxIterations=iters, convergenceThreshold=th)
    _same_regions(ctx.detect_affine_shape(dimgs[0], regs[0], par), want, "iters %d th %g" % (iters, th))


def test_no_iterations_no_launch(ctx, modsx, dimgs):
    before = ctx.affshape_counters()
    regs = AC.regions()[0]
    par = modsx.default_affshape_params(maxIterations=0)
    assert len(ctx.detect_affine_shape(dimgs[0], regs, par)) == 0
    assert len(ctx.detect_affine_shape(dimgs[0], regs[:0])) == 0
    got = ctx.debug_affine_shape([dimgs[0]], [regs], par)
    assert (got["ok"] == 0).all() and (got["iters"][~got["border"]] == 0).all() and (got["iters"][got["border"]] == -1).all()
    assert (got["u"] == np.array([1, 0, 0, 1], np.float32)).all()
    after = ctx.affshape_counters()
    assert after["launches"] == before["launches"] and after["launched"] == before["launched"]


# --------------------------------------------------------------------------------------------------------------- 5. batch
def test_batch_equals_single_calls(ctx, modsx, oracle, dimgs):
    regs = AC.regions()
    exp = AC.expected(oracle)
    singles = [ctx.detect_affine_shape(im, r) for im, r in zip(dimgs, regs)]
    batch = ctx.detect_affine_shape_batch(dimgs, regs)
    assert len(batch) == 3
    for i in range(3):
        _same_regions(batch[i], singles[i], "batch against single, image %d" % i)
        _same_regions(batch[i], exp[i][0], "batch against the model, image %d" % i)
    # an image without regions and one whose regions are all refused, between two ordinary ones
    refused = regs[2][exp[2][1]["border"]]
    assert len(refused) >= 10
    lists = [regs[0], regs[1][:0], refused, regs[1]]
    ims = [dimgs[0], dimgs[1], dimgs[2], dimgs[1]]
    got = ctx.detect_affine_shape_batch(ims, lists)
    assert [len(g) for g in got] == [len(exp[0][0]), 0, 0, len(exp[1][0])]
    _same_regions(got[0], exp[0][0], "mixed batch, image 0")
    _same_regions(got[3], exp[1][0], "mixed batch, image 3")
    assert len(ctx.detect_affine_shape_batch([dimgs[2]], [refused])[0]) == 0          # nothing to launch at all
    assert ctx.detect_affine_shape_batch([], []) == []
    dbg = ctx.debug_affine_shape(ims, lists)
    assert dbg["launched"] == int((~exp[0][1]["border"]).sum() + (~exp[1][1]["border"]).sum())


# ------------------------------------------------------------------------------------------------------ 6. shared context
def test_shared_context_with_the_detector(modsx, oracle, small_pair):
    """detect_affine_keypoints, detect_affine_shape, detect_affine_keypoints on ONE context against the same calls on fresh
    contexts: the external launch clears the queue's counters itself and leaves numbers in them, and the detector's next launch
    must find its own zeros (scan_extrema's fill)."""
    img = small_pair[0]
    par = modsx.default_hessaff_params()
    regs, plane = AC.regions()[0], AC.images(oracle)[0]

    def fresh(fn):
        c = modsx.Context(0)
        try:
            return fn(c)
        finally:
            c.close()

    def detect(c):
        im = c.upload(img)
        try:
            return c.detect_affine_keypoints(im, par)
        finally:
            im.free()

    def adapt(c):
        im = c.upload(plane)
        try:
            return c.detect_affine_shape(im, regs)
        finally:
            im.free()

    want_k, want_r = fresh(detect), fresh(adapt)
    assert len(want_k) > 100
    _same_regions(want_r, AC.expected(oracle)[0][0], "fresh context")

    def interleaved(c):
        return detect(c), adapt(c), detect(c), adapt(c)

    k1, r1, k2, r2 = fresh(interleaved)
    assert same_records(k1, want_k) and same_records(k2, want_k)
    _same_regions(r1, want_r, "after one detection")
    _same_regions(r2, want_r, "after two detections")
    k3, r3 = fresh(lambda c: (adapt(c), detect(c)))[::-1]
    assert same_records(k3, want_k)
    _same_regions(r3, want_r, "before any detection")


# ------------------------------------------------------------------------------------------------------------ 7. counters
def test_counters(modsx, oracle):
    c = modsx.Context(0)
    ims = [c.upload(p) for p in AC.images(oracle)]
    try:
        assert c.affshape_counters() == dict(calls=0, regions=0, border_refused=0, launched=0, converged=0, launches=0)
        regs, exp = AC.regions(), AC.expected(oracle)
        c.detect_affine_shape(ims[0], regs[0])
        n0, b0, k0 = len(regs[0]), int(exp[0][1]["border"].sum()), len(exp[0][0])
        assert c.affshape_counters() == dict(calls=1, regions=n0, border_refused=b0, launched=n0 - b0, converged=k0, launches=1)
        c.detect_affine_shape_batch(ims, regs)             # one launch for the three images
        n = sum(len(r) for r in regs)
        b = sum(int(e[1]["border"].sum()) for e in exp)
        k = sum(len(e[0]) for e in exp)
        assert c.affshape_counters() == dict(calls=2, regions=n0 + n, border_refused=b0 + b, launched=n0 - b0 + n - b,
                                             converged=k0 + k, launches=2)
        c.detect_affine_shape(ims[0], regs[0][:0])         # returns before the engine
        c.detect_affine_shape(ims[2], regs[2][exp[2][1]["border"]])        # a call without a launch
        got = c.affshape_counters()
        assert got["calls"] == 3 and got["launches"] == 2 and got["border_refused"] == b0 + b + int(exp[2][1]["border"].sum())
    finally:
        for im in ims:
            im.free()
        c.close()


# --------------------------------------------------------------------------------------------------------- the SURF chain
def test_surf_chain_on_the_small_cat_pair(ctx, modsx, oracle, cat_pair):
    """detect_surf -> surf_regions -> detect_affine_shape -> detect_orientation -> (identity reprojection) -> describe_regions ->
    match_fginn on the cat pair at half size: the reference's SURF branch with doBaumberg = 1 (imagerepresentation.cpp:1048,
    1226-1236), against the same chain with tests/surfdet_model.py in step 1, tests/affshape_model.py in step 3 and the oracle in
    the others.  SURF scales are f32 numbers widened to double, so the model takes them."""
    import surfdet_cases as SC
    import surfdet_model as SD
    sides = []
    for k, g in enumerate([np.ascontiguousarray(oracle.gray_from_bgr(c)[::2, ::2]) for c in cat_pair[:2]]):
        pts = SD.detect(g, **SC.INI)["points"]
        want = np.zeros(len(pts), modsx.REGION)
        want["det_kp"] = SD.keypoints(pts, modsx.KEYPOINT)
        want["type"], want["id"], want["img_id"] = SD.DET_SURF, np.arange(len(pts)), k
        want_a, rep = AM.run(oracle, g, want)
        assert 0.3 * len(want) < len(want_a) < len(want)                     # the stage keeps some and drops some
        want_r = oracle.reproject_regions(oracle.detect_orientation(g, want_a), np.eye(3), g.shape[1], g.shape[0])
        want_d = oracle.describe_regions(g, want_r)
        im = ctx.upload(g)
        try:
            regs = modsx.surf_regions(ctx.detect_surf(im), img_id=k)
            adapted = ctx.detect_affine_shape(im, regs)
            ro = modsx.reproject_regions(ctx.detect_orientation(im, adapted), np.eye(3), g.shape[1], g.shape[0])
            desc = ctx.describe_regions(im, ro)
        finally:
            im.free()
        _same_regions(adapted, want_a, "adapted SURF regions of image %d" % k)
        assert len(ro) == len(want_r) > 20 and same_records(ro, want_r)
        assert desc.tobytes() == want_d.tobytes()
        sides.append((ro, desc, want_r, want_d))
    (r1, d1, w1, m1), (r2, d2, w2, m2) = sides
    pos2 = np.stack([w2["reproj_kp"]["x"], w2["reproj_kp"]["y"]], 1)
    tent = oracle.match_fginn(m1, m2, pos2, 0.8, 30.0, 50)
    got = ctx.match_fginn(d1, d2, np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1), 0.8, 30.0, 50)
    assert len(tent) > 0, "a chain without a tentative compares empty lists"
    assert same_records(got, tent)


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(ctx, modsx, oracle, dimgs):
    regs = np.array(AC.regions()[0][:20])
    for kw in (dict(smmWindowSize=4), dict(smmWindowSize=21), dict(smmWindowSize=1), dict(affBmbrgMethod=1)):
        with pytest.raises(RuntimeError):
            ctx.detect_affine_shape(dimgs[0], regs, modsx.default_affshape_params(**kw))
        with pytest.raises(RuntimeError):
            ctx.debug_affine_shape([dimgs[0]], [regs], modsx.default_affshape_params(**kw))
    for f, v in (("x", np.nan), ("s", np.inf), ("a21", -np.inf), ("s", 1e12)):
        bad = regs.copy()
        bad["det_kp"][f][7] = v
        with pytest.raises(RuntimeError):
            ctx.detect_affine_shape(dimgs[0], bad)
        with pytest.raises(RuntimeError):
            ctx.detect_affine_shape_batch([dimgs[1], dimgs[0]], [regs, bad])
    with pytest.raises(RuntimeError):           # k_baumberg<19> has no other window
        ctx.debug_affine_shape([dimgs[0]], [regs], modsx.default_affshape_params(smmWindowSize=11), variant=1)
    with pytest.raises(RuntimeError):
        ctx.debug_affine_shape([dimgs[0]], [regs], variant=4)
    tiny = ctx.upload(np.zeros((3, 8), np.float32))
    try:
        with pytest.raises(RuntimeError, match="4 x 4"):
            ctx.detect_affine_shape(tiny, regs)
    finally:
        tiny.free()
    _same_regions(ctx.detect_affine_shape(dimgs[0], AC.regions()[0]), AC.expected(oracle)[0][0], "after the refusals")
