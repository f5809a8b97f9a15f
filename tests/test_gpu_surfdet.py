"""GPU: the SURF detector, bit for bit against tests/surfdet_model.py -- the restatement of OpenSURF's FastHessian that
tests/test_surfdet_model_cpu.py ties to the compiled reference -- on the images and parameter sets of tests/surfdet_cases.py:
every stage of the debug tap, the point list and its order, the batch against single calls on one context and on a fresh one, the
point buffer's regrow, the refusals, and the chain detect_surf -> surf_regions -> describe_regions_surf -> match_regions_f32."""
import ctypes as C

import numpy as np
import pytest

import fginn32_cases as FC
import surf_model as SM
import surfdet_cases as SC
import surfdet_model as M

pytestmark = pytest.mark.gpu

CHAIN_MR = 20.5                # the mrSize of the SURF descriptor chain in tests/test_gpu_surf.py: finite rows on real patches


def same_bits(got, ref, what=""):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero(got.reshape(-1).view(np.uint8 if got.itemsize == 1 else "u%d" % got.itemsize) !=
                         ref.reshape(-1).view(np.uint8 if ref.itemsize == 1 else "u%d" % ref.itemsize))[0]
        raise AssertionError("%s: %d of %d values differ, first at %d: %r != %r" %
                             (what, len(bad), got.size, bad[0], got.reshape(-1)[bad[0]], ref.reshape(-1)[bad[0]]))


def same_keypoints(modsx, got, points, what=""):
    want = M.keypoints(points, modsx.KEYPOINT)
    assert got.dtype == want.dtype
    assert len(got) == len(want), (what, len(got), len(want))
    for f in got.dtype.names:                             # every field as bits, the -0.0 of a21 included
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


def params(modsx, par):
    return modsx.surfdet_params(**par)


@pytest.mark.parametrize("name", SC.names())
def test_every_stage_and_the_points(ctx, modsx, name):
    _, img, par = SC.case(name)
    m = SC.model(name)
    im = ctx.upload(img)
    try:
        tap = ctx.debug_surfdet(im, params(modsx, par))
        kps = ctx.detect_surf(im, params(modsx, par))
    finally:
        im.free()
    assert np.array_equal(tap["layers"], np.array(m["layers"], np.int32))
    same_bits(tap["integral"], m["integral"], "integral image")
    for k in range(len(m["layers"])):
        same_bits(tap["resp"][k], m["resp"][k], "responses of layer %d" % k)
        same_bits(tap["lap"][k], m["lap"][k], "laplacian of layer %d" % k)
    same_bits(tap["extrema"], m["extrema"], "extremum list")
    for key in ("dD", "H", "x"):
        same_bits(tap[key], m[key], key)
    assert np.array_equal(tap["accepted"], m["accepted"]) and np.array_equal(tap["laplacian"], m["laplacian"])
    same_keypoints(modsx, kps, m["points"], name)
    # the accepted extrema are the points, in order
    assert len(kps) == int(tap["accepted"].sum())


def test_flat_image_gives_no_point(ctx, modsx):
    for name in ("flat_320x240",):
        _, img, par = SC.case(name)
        im = ctx.upload(img)
        try:
            assert len(ctx.detect_surf(im, params(modsx, par))) == 0
            assert len(ctx.debug_surfdet(im, params(modsx, par))["extrema"]) == 0
        finally:
            im.free()


def _batch_cases():
    return [SC.case(n) for n in SC.BATCH]


def test_batch_equals_single_calls_on_this_and_on_a_fresh_context(ctx, modsx):
    par = params(modsx, SC.INI)
    cases = _batch_cases()
    assert len({c[1].shape for c in cases}) == 3
    want = [SC.model_of(img, **SC.INI)["points"] for _, img, _ in cases]
    assert sum(len(w) for w in want) > 0
    fresh = modsx.Context(0)
    try:
        for c in (ctx, fresh):
            ims = [c.upload(img) for _, img, _ in cases]
            try:
                before = c.surfdet_counters()
                got = c.detect_surf_batch(ims, par)
                d = {k: v - before[k] for k, v in c.surfdet_counters().items()}
                assert d["calls"] == 1 and d["images"] == 3 and d["accepted"] == sum(len(w) for w in want), d
                singles = [c.detect_surf(im, par) for im in ims]
                # the same list once more, reversed: the tables of the second set are not those of the first
                back = c.detect_surf_batch(ims[::-1], par)[::-1]
                assert c.detect_surf_batch([], par) == []
            finally:
                for im in ims:
                    im.free()
            for g, s, b, w, (name, _, _) in zip(got, singles, back, want, cases):
                same_keypoints(modsx, g, w, "batch, " + name)
                same_keypoints(modsx, s, w, "single, " + name)
                same_keypoints(modsx, b, w, "reversed batch, " + name)
    finally:
        fresh.close()


def test_more_images_than_one_launch_set(ctx, modsx):
    """34 images of three sizes: two launch sets (the library takes 32 at a time)"""
    par = params(modsx, SC.INI)
    cases = [SC.case(n) for n in ("s63x48", "s65x48", "s129x48")]
    ims = [ctx.upload(img) for _, img, _ in cases]
    try:
        order = [k % 3 for k in range(34)]
        got = ctx.detect_surf_batch([ims[k] for k in order], par)
    finally:
        for im in ims:
            im.free()
    for k, g in zip(order, got):
        same_keypoints(modsx, g, SC.model_of(cases[k][1], **SC.INI)["points"], "image %d" % k)


def test_thresh_zero_regrows_the_point_buffer_once(modsx):
    """thresh = 0 on the 320 x 240 dots at init_sample 1: more points than a fresh context's buffer holds.  The first call grows
    it, the second finds room; both return every point of the model."""
    name = "dots320x240_is1_t0"
    _, img, par = SC.case(name)
    m = SC.model(name)
    assert len(m["points"]) > 500 and len(m["extrema"]) > len(m["points"])
    c = modsx.Context(0)
    try:
        im = c.upload(img)
        small = c.upload(SC.case("s65x48")[1])
        assert len(c.detect_surf(small, params(modsx, SC.INI))) == len(SC.model("s65x48")["points"])
        assert c.surfdet_counters()["regrows"] == 0
        first = c.detect_surf(im, params(modsx, par))
        c1 = c.surfdet_counters()
        second = c.detect_surf(im, params(modsx, par))
        c2 = c.surfdet_counters()
        im.free(); small.free()
    finally:
        c.close()
    same_keypoints(modsx, first, m["points"], "first call")
    same_keypoints(modsx, second, m["points"], "second call")
    assert c1["regrows"] == 1 and c2["regrows"] == 1, (c1, c2)
    assert c2["accepted"] - c1["accepted"] == len(m["points"]) and c2["extrema"] - c1["extrema"] == len(m["extrema"])
    assert c2["calls"] == 3 and c2["images"] == 3


def test_refusals_leave_the_context_usable(ctx, modsx):
    L = modsx.lib()
    par = params(modsx, SC.INI)
    out, cnt = C.c_void_p(), (C.c_int * 2)()
    _, img, _ = SC.case("s65x48")
    im = ctx.upload(img)
    tiny = ctx.upload(np.full((12, 40), 100.0, np.float32))          # 12 / 2 / 8 == 0: octave 4 has no rows
    try:
        before = ctx.surfdet_counters()
        ptrs = (C.c_void_p * 2)(im.h, tiny.h)
        assert L.modsx_detect_surf(ctx._c(), None, C.byref(par), C.byref(out)) == -1
        assert L.modsx_detect_surf(ctx._c(), C.c_void_p(im.h), None, C.byref(out)) == -1
        assert L.modsx_detect_surf(ctx._c(), C.c_void_p(im.h), C.byref(par), None) == -1
        assert L.modsx_detect_surf_batch(ctx._c(), ptrs, -1, C.byref(par), C.byref(out), cnt) == -1
        assert L.modsx_detect_surf_batch(ctx._c(), None, 2, C.byref(par), C.byref(out), cnt) == -1
        assert L.modsx_detect_surf_batch(ctx._c(), ptrs, 2, C.byref(par), C.byref(out), None) == -1
        assert L.modsx_detect_surf_batch(ctx._c(), (C.c_void_p * 2)(im.h, None), 2, C.byref(par), C.byref(out), cnt) == -1
        assert L.modsx_detect_surf(ctx._c(), C.c_void_p(tiny.h), C.byref(par), C.byref(out)) == -1
        assert b"width or height 0" in L.modsx_last_error()
        assert L.modsx_detect_surf_batch(ctx._c(), ptrs, 2, C.byref(par), C.byref(out), cnt) == -1      # one bad image refuses the set
        with pytest.raises(RuntimeError):
            ctx.debug_surfdet(tiny, par)
        assert ctx.surfdet_counters() == before                                                         # nothing was launched
        # the same image is fine with one octave, and an empty batch succeeds
        assert len(ctx.detect_surf(tiny, modsx.surfdet_params(octaves=1))) == 0
        assert L.modsx_detect_surf_batch(ctx._c(), None, 0, C.byref(par), C.byref(out), None) == 0
        L.modsx_free(out)
        same_keypoints(modsx, ctx.detect_surf(im, par), SC.model("s65x48")["points"], "after the refusals")
    finally:
        im.free(); tiny.free()


def _small_cat(oracle, cat_pair):
    return [np.ascontiguousarray(oracle.gray_from_bgr(g)[::2, ::2]) for g in cat_pair[:2]]


def test_chain_on_the_small_cat_pair(ctx, modsx, oracle, cat_pair):
    """detect_surf -> surf_regions -> (identity reprojection) -> describe_regions_surf -> match_regions_f32 at dim 64 on the cat pair
    at half size, against the same chain fed with the model's points, the oracle's patches and the rows of tests/surf_model.py"""
    par = modsx.default_pair_params(ransac_seed=1)
    sides = []
    for k, g in enumerate(_small_cat(oracle, cat_pair)):
        pts = M.detect(g, **SC.INI)["points"]
        want_regs = np.zeros(len(pts), modsx.REGION)
        want_regs["det_kp"] = M.keypoints(pts, modsx.KEYPOINT)
        want_regs["type"], want_regs["id"], want_regs["img_id"] = M.DET_SURF, np.arange(len(pts)), k
        want_regs = modsx.reproject_regions(want_regs, np.eye(3), g.shape[1], g.shape[0])
        pats = [oracle.describe_patch(oracle.extract_patch(g, want_regs[i:i + 1], mr_size=CHAIN_MR), photo_norm=1)[1].reshape(41, 41)
                for i in range(len(want_regs))]
        want = SM.describe(pats, CHAIN_MR)
        im = ctx.upload(g)
        try:
            kps = ctx.detect_surf(im)
            regs = modsx.reproject_regions(modsx.surf_regions(kps, img_id=k), np.eye(3), g.shape[1], g.shape[0])
            desc = ctx.describe_regions_surf(im, regs, mr_size=CHAIN_MR)
        finally:
            im.free()
        same_keypoints(modsx, kps, pts, "image %d" % k)
        assert len(regs) > 20 and len(regs) == len(want_regs)
        for f in ("img_id", "img_reproj_id", "id", "parent_id", "type"):
            assert np.array_equal(regs[f], want_regs[f]), f
        for kp in ("det_kp", "reproj_kp"):
            for f in modsx.KEYPOINT.names:
                assert regs[kp][f].tobytes() == want_regs[kp][f].tobytes(), (kp, f)
        assert np.isfinite(want).all()
        same_bits(desc, want, "SURF rows of image %d" % k)
        sides.append((regs, desc, want))
    (r1, d1, m1), (r2, d2, m2) = sides
    got = ctx.match_regions_f32(r1, d1, r2, d2, par)
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    tent = oracle.match_fginn(m1, m2, pos2, par.match_ratio, par.contradDist, par.nn)
    p4 = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                   r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = oracle.duplicate_filtering(p4, tent["ratio"], par.duplicateDist, True)
    assert len(tent) > 0, "a chain without a tentative compares empty lists"
    assert got["n_regions"] == (len(r1), len(r2)) and got["n_tentatives"] == len(tent)
    FC.same_tents(got["tentatives"], tent[order[keep]])
