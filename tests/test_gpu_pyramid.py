"""GPU: the scale-space front end (kernels_pyramid.hip driven by engine_detect.hip) against the oracle, level by level and
extremum by extremum, on the inputs of tests/pyramid_cases.py; tests/test_pyramid_cases_cpu.py proves what those inputs reach.
Bar: bit-exact.  Which kernel and which path ran is read from Context.detect_counters() (differences of two readings), and a
test fails when the counters show another path than the one its case names.

  - blur: every instantiated half width R = 1 .. 8 on shapes around the tile edges; 32-row and 16-row tiles on both sides of the
    2560-tile rule, plain and with the fused Hessian; the refusal of a 19-tap kernel;
  - debug_pyramids: a batch of four sizes, every plane of every octave, against gaussian_blur -> octave_levels -> resize_half;
  - debug_scan_levels: the planted planes through the per-octave and the per-level scan kernel (the latter also for L = 5, in a
    child process under MODSX_NMS_PER_LEVEL), raw candidates and claimed keypoints;
  - the host tail: the second copy of a candidate set larger than the speculative download on a fresh context, the flush of a
    full job table;
  - border < 1 is refused before anything is launched.
The queue-overflow error (more than 2^21 candidates in one set) is not aimed at: no small input reaches it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pyramid_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

BLUR_R = tuple("blur_r%d" % r for r in range(1, 9))


def _moved(ctx, fn):
    """fn()'s result and what every counter moved by"""
    before = ctx.detect_counters()
    out = fn()
    after = ctx.detect_counters()
    return out, {k: after[k] - before[k] for k in after}


def _launches(d):
    """the non-zero launch counters of a difference"""
    return {k: v for k, v in d.items() if v and not k.startswith("last_")}


@pytest.fixture(scope="module")
def scans(oracle):
    return {c.name: PC.oracle_scan(oracle, c) for c in PC.SCAN_CASES}


# ---- blur ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", range(1, 9))
def test_blur_every_half_width_on_shapes_around_the_tile_edges(ctx, oracle, R):
    sigma = PC.BLUR_SIGMAS[R - 1]
    n = 0
    for rows in PC.BLUR_ROWS:
        for cols in PC.BLUR_COLS:
            img = PC.image(rows, cols, 100 * R + n)
            im = ctx.upload(img)
            got, d = _moved(ctx, lambda: ctx.gaussian_blur(im, sigma))
            im.free()
            assert _launches(d) == {"blur_th16": 1, "blur_r%d" % R: 1}, (rows, cols, d)
            assert np.array_equal(got, oracle.gaussian_blur(img, sigma)), (rows, cols)
            n += 1


def test_blur_with_19_taps_is_refused(ctx):
    im = ctx.upload(PC.image(33, 65, 1))
    before = ctx.detect_counters()
    with pytest.raises(RuntimeError, match="ksize > 17"):
        ctx.gaussian_blur(im, PC.REFUSED_SIGMA)
    assert ctx.detect_counters() == before
    im.free()


@pytest.fixture(scope="module")
def boundary_images():
    return {32: PC.image(PC.TILE32_SHAPE[0], PC.TILE32_SHAPE[1], 11), 16: PC.image(PC.TILE16_SHAPE[0], PC.TILE16_SHAPE[1], 12)}


@pytest.mark.parametrize("th,sigma", [(32, s) for s in PC.TILE32_BLUR_SIGMAS] + [(16, s) for s in PC.TILE16_BLUR_SIGMAS])
def test_blur_on_both_sides_of_the_tile_height_rule(ctx, oracle, boundary_images, th, sigma):
    img = boundary_images[th]
    im = ctx.upload(img)
    got, d = _moved(ctx, lambda: ctx.gaussian_blur(im, sigma))
    im.free()
    assert _launches(d) == {"blur_th%d" % th: 1, "blur_r%d" % (PC.BLUR_SIGMAS.index(sigma) + 1): 1}
    assert np.array_equal(got, oracle.gaussian_blur(img, sigma))


@pytest.mark.parametrize("th", [32, 16])
def test_octave_levels_on_both_sides_of_the_tile_height_rule(ctx, modsx, oracle, boundary_images, th):
    img = boundary_images[th]
    im = ctx.upload(img)
    (blurs, resps), d = _moved(ctx, lambda: ctx.octave_levels(im, modsx.default_hessaff_params()))
    im.free()
    # the first level is given (its Hessian from the stand-alone kernel), the four others are blur launches of R = 4 .. 7
    assert _launches(d) == {"blur_th%d" % th: 4, "hessian": 1, "blur_r4": 1, "blur_r5": 1, "blur_r6": 1, "blur_r7": 1}
    rb, rr = oracle.octave_levels(img, oracle.default_params())
    assert np.array_equal(blurs, rb)
    assert np.array_equal(resps[:, 1:-1, 1:-1], rr[:, 1:-1, 1:-1])
    assert not resps[:, 0, :].any() and not resps[:, -1, :].any() and not resps[:, :, 0].any() and not resps[:, :, -1].any()


# ---- pyramids of a batch ------------------------------------------------------------------------------------------------------------
def test_debug_pyramids_mixed_batch_every_plane(ctx, modsx, oracle):
    imgs = PC.mixed_batch()
    ims = [ctx.upload(a) for a in imgs]
    p, po = modsx.default_hessaff_params(), oracle.default_params()
    got, d = _moved(ctx, lambda: ctx.debug_pyramids(ims, p))
    for im in ims:
        im.free()
    # octave 0: the first-level blur and four levels on 32-row tiles; octaves 1 and 2: a resize and four levels on 16-row tiles
    assert _launches(d) == {"blur_th32": 5, "blur_th16": 8, "resize": 2, "blur_r4": 3, "blur_r5": 4, "blur_r6": 3, "blur_r7": 3}
    L = p.numberOfScales + 2
    for i, img in enumerate(imgs):
        shapes = PC.octave_shapes(img.shape[0], img.shape[1], po.border)
        assert [b.shape[1:] for b, _ in got[i]] == shapes, i
        first = oracle.gaussian_blur(img, float(np.sqrt(np.float32(po.initialSigma) ** 2 - np.float32(0.25))))
        for o, (blurs, resps) in enumerate(got[i]):
            rb, rr = oracle.octave_levels(first, po, nlevels=L)
            assert np.array_equal(blurs, rb), (i, o)
            assert np.array_equal(resps[:, 1:-1, 1:-1], rr[:, 1:-1, 1:-1]), (i, o)
            assert not resps[:, 0, :].any() and not resps[:, -1, :].any() and not resps[:, :, 0].any() and not resps[:, :, -1].any()
            first = oracle.resize_half(rb[po.numberOfScales])


# ---- extrema scan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.SCAN_CASES, ids=repr)
def test_debug_scan_levels_every_extremum(ctx, modsx, scans, case):
    assert not os.environ.get("MODSX_NMS_PER_LEVEL")
    bad = PC.run_scan_case(ctx, modsx, case, scans[case.name])
    assert bad == []


def test_debug_scan_levels_per_level_kernel_for_five_planes():
    """MODSX_NMS_PER_LEVEL=1 sends L = 5 through k_nms_localize as well.  A child process: this session's library keeps its default."""
    code = (
        "import sys, json\n"
        "sys.path.insert(0, %r)\n"
        "import mods_amd\n"
        "from oracle import pyoracle as O\n"
        "from tests import pyramid_cases as PC\n"
        "ctx = mods_amd.Context(0)\n"
        "res = {}\n"
        "for case in PC.SCAN_CASES:\n"
        "    if case.L == 5:\n"
        "        res[case.name] = PC.run_scan_case(ctx, mods_amd, case, PC.oracle_scan(O, case), per_level=True)\n"
        "ctx.close()\n"
        "print(json.dumps(res))\n"
    ) % (ROOT,)
    env = dict(os.environ, MODSX_NMS_PER_LEVEL="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == sum(c.L == 5 for c in PC.SCAN_CASES) >= 10
    assert all(v == [] for v in res.values()), res


# ---- host tail ----------------------------------------------------------------------------------------------------------------------
def test_fresh_context_copies_a_large_candidate_set_twice(modsx, scans):
    """A fresh context copies 1024 records speculatively: a set with more costs exactly one second copy of them all, and a smaller
    set after it none."""
    c = modsx.Context(0)
    try:
        assert c.detect_counters()["second_copies"] == 0
        big = PC.scan_case(PC.BIG)
        assert PC.run_scan_case(c, modsx, big, scans[big.name]) == []
        assert c.detect_counters()["second_copies"] == 1
        small = PC.scan_case("plateau")
        assert PC.run_scan_case(c, modsx, small, scans[small.name]) == []
        assert c.detect_counters()["second_copies"] == 1
    finally:
        c.close()


def test_full_job_table_is_flushed(ctx, modsx, oracle):
    imgs = PC.flush_batch()
    ims = [ctx.upload(a) for a in imgs]
    got, d = _moved(ctx, lambda: ctx.debug_detect_scalespace_batch(ims, modsx.default_hessaff_params(**PC.FLUSH_PARAMS)))
    for im in ims:
        im.free()
    total, flushed = PC.flush_jobs()
    assert d["nms_flushes"] == 1 and d["scan_per_level"] == 2 and d["scan_per_octave"] == 0
    assert ctx.detect_counters()["last_jobs"] == total > PC.NMS_MAXJ
    po = oracle.default_params(**PC.FLUSH_PARAMS)
    behind = 0
    for i, img in enumerate(imgs):
        ref = oracle.detect_scalespace(img, po)
        assert len(got[i]) == len(ref), i
        for f in PC.SSKP_FIELDS:
            assert np.array_equal(got[i][f], ref[f]), (i, f)
        behind += int(((ref["octave"] == 6) | ((ref["octave"] == 5) & (i >= 10))).sum())
    assert behind >= 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [0, -1])
def test_border_below_one_is_refused_before_any_launch(ctx, modsx, border):
    p = modsx.default_hessaff_params(border=border)
    im = ctx.upload(PC.image(48, 64, 2))
    resp, blur = PC.scan_case("plateau").planes()
    before = ctx.detect_counters()
    for call in (lambda: ctx.detect_scalespace(im, p), lambda: ctx.detect_affine_keypoints(im, p), lambda: ctx.octave_levels(im, p),
                 lambda: ctx.debug_pyramids([im], p), lambda: ctx.debug_scan_levels(resp, blur, p),
                 lambda: ctx.debug_detect_scalespace_batch([im, im], p)):
        with pytest.raises(RuntimeError, match="border must be at least 1"):
            call()
    assert ctx.detect_counters() == before
    im.free()
    # the context still works
    im = ctx.upload(PC.image(48, 64, 2))
    ctx.detect_scalespace(im, modsx.default_hessaff_params())
    im.free()
