"""GPU: the three Baumberg kernels (mods_amd/csrc/kernels_affine.hip: k_baumberg_stream, k_baumberg<19>, k_baumberg<0>) against the
oracle's findAffineShape, keypoint by keypoint, through Context.debug_baumberg.

Comparison rule, everywhere: the shape u[4], ok and iters of EVERY job are bit-equal to oracle.find_affine_shape_batch -- failed
keypoints included, with the state and the loop counter at the moment they left -- and no job is left unwritten (the entry fills
the result buffer with 0xFF bytes: iters == -1).  No tolerance: same operands, same order, no contraction.

The jobs are those of tests/baumberg_cases.py; tests/test_baumberg_cases_cpu.py proves without a device that they reach every
exit, every class of border contact and, at chunk lengths 3, 5 and 8, every refill pattern of the stream kernel's two slots.
  1. stream kernel, whole list, chunk 0 (the production rule), 1 (the second slot never fills), 2, 3, 5, 8, 13
  2. prefixes of the list (odd tails, chunk counts that are no multiple of 8, padded grids), and n = 0
  3. k_baumberg<19> and k_baumberg<0> at W = 19 on the whole list
  4. k_baumberg<0> at every other odd window from 3 to 17
  5. iteration caps, convergence thresholds and initial sigmas, stream kernel at chunk 3
  6. one context at W = 19, 11 and 19 again (the window mask is uploaded again)
  7. the entry is the production path: modsx_detect_affine_keypoints rebuilt from detect_scalespace + debug_baumberg
"""
import numpy as np
import pytest

from tests import baumberg_cases as BC
from tests.common import same_records

pytestmark = pytest.mark.gpu

IDENT = np.array([1, 0, 0, 1], np.float32)


@pytest.fixture(scope="module")
def dplanes(ctx, oracle):
    ims = [ctx.upload(p) for p in BC.planes(oracle)]     # f32, 1 channel: stored unchanged
    yield ims
    for im in ims:
        im.free()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare(got, ref, what):
    n = len(ref["ok"])
    assert len(got["ok"]) == n
    unwritten = np.nonzero(got["iters"] == -1)[0]
    assert len(unwritten) == 0, (what, "jobs no wavefront wrote", unwritten[:10])
    bad = np.nonzero((got["ok"] != ref["ok"]) | (got["iters"] != ref["iters"]) | (_bits(got["u"]) != _bits(ref["u"])).any(1))[0]
    if len(bad):
        k = int(bad[0])
        detail = dict(job=k, got=(got["u"][k].tolist(), int(got["ok"][k]), int(got["iters"][k])),
                      ref=(ref["u"][k].tolist(), int(ref["ok"][k]), int(ref["iters"][k]), BC.REASONS[int(ref["reason"][k])]))
        raise AssertionError("%s: %d of %d keypoints differ from the oracle, first %r" % (what, len(bad), n, detail))


def _run(ctx, modsx, oracle, dplanes, plane_of, xyspd, variant=0, chunk=0, **params):
    ref = BC.oracle_results(oracle, plane_of, xyspd, **params)
    got = ctx.debug_baumberg(dplanes, plane_of, xyspd, modsx.default_hessaff_params(**params), variant=variant, chunk=chunk)
    W = params.get("smmWindowSize", 19)
    assert got["geometry"] == modsx.baumberg_geometry(len(plane_of), W, variant, chunk)
    _compare(got, ref, "variant %d chunk %d %r" % (variant, chunk, params))
    return got


@pytest.mark.parametrize("chunk", [0, 1, 2, 3, 5, 8, 13])
def test_stream_kernel_whole_list(ctx, modsx, oracle, dplanes, chunk):
    po, xy = BC.jobs()
    g = _run(ctx, modsx, oracle, dplanes, po, xy, chunk=chunk)["geometry"]
    want = chunk if chunk else 2
    assert (g["kernel"], g["chunk"], g["nchunks"]) == (0, want, (len(po) + want - 1) // want)     # the chunk was really taken


@pytest.mark.parametrize("chunk", [2, 3, 8])
def test_stream_kernel_prefixes(ctx, modsx, oracle, dplanes, chunk):
    for n in (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200):
        po, xy = BC.subset(n)
        g = _run(ctx, modsx, oracle, dplanes, po, xy, chunk=chunk)["geometry"]
        assert g["chunk"] == chunk and g["nchunks"] == (n + chunk - 1) // chunk and g["grid"] == 8 * ((g["nchunks"] + 7) // 8)


def test_no_jobs_no_launch(ctx, modsx, dplanes):
    for variant, chunk in ((0, 0), (0, 3), (1, 0), (2, 0)):
        got = ctx.debug_baumberg(dplanes, np.zeros(0, np.int32), np.zeros((0, 4), np.float32), modsx.default_hessaff_params(),
                                 variant=variant, chunk=chunk)
        assert len(got["ok"]) == 0 and got["geometry"]["nchunks"] == 0 and got["geometry"]["grid"] == 0


@pytest.mark.parametrize("variant", [1, 2])
def test_one_keypoint_kernels_whole_list(ctx, modsx, oracle, dplanes, variant):
    po, xy = BC.jobs()
    g = _run(ctx, modsx, oracle, dplanes, po, xy, variant=variant)["geometry"]
    assert g == dict(kernel=variant, chunk=1, nchunks=len(po), grid=len(po))


@pytest.mark.parametrize("W", [3, 5, 7, 9, 11, 13, 15, 17])
def test_any_window_kernel(ctx, modsx, oracle, dplanes, W):
    po, xy = BC.subset(300)
    g = _run(ctx, modsx, oracle, dplanes, po, xy, variant=2, smmWindowSize=W)["geometry"]
    assert g["kernel"] == 2
    assert modsx.baumberg_geometry(300, W, 0, 0) == g         # ... which is what production launches at this window


@pytest.mark.parametrize("sigma", [0.8, 1.6])
@pytest.mark.parametrize("th", [0.01, 0.05, 0.3])
@pytest.mark.parametrize("iters", [0, 1, 2, 16])
def test_parameter_sweep_stream_kernel(ctx, modsx, oracle, dplanes, iters, th, sigma):
    po, xy = BC.jobs()
    got = _run(ctx, modsx, oracle, dplanes, po, xy, chunk=3, maxIterations=iters, convergenceThreshold=th, affInitialSigma=sigma)
    if iters == 0:
        assert (got["iters"] == 0).all() and (got["ok"] == 0).all() and (got["u"] == IDENT).all()


def test_window_mask_follows_the_window_size(ctx, modsx, oracle, dplanes):
    po, xy = BC.subset(300)
    for W in (19, 11, 19):
        _run(ctx, modsx, oracle, dplanes, po, xy, smmWindowSize=W)


def test_out_of_contract_jobs_are_refused(ctx, modsx, dplanes):
    par = modsx.default_hessaff_params()
    ok = [20.0, 20.0, 1.6, 1.0]
    for col, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, 0.0), (3, -1.0), (3, np.nan)):
        row = list(ok)
        row[col] = v
        with pytest.raises(RuntimeError):
            ctx.debug_baumberg(dplanes, [0, 0], [ok, row], par)
    with pytest.raises(RuntimeError):
        ctx.debug_baumberg(dplanes, [len(dplanes)], [ok], par)
    with pytest.raises(RuntimeError):       # k_baumberg<19> has no other window
        ctx.debug_baumberg(dplanes, [0], [ok], modsx.default_hessaff_params(smmWindowSize=11), variant=1)
    tiny = ctx.upload(np.zeros((3, 8), np.float32))
    try:
        with pytest.raises(RuntimeError):
            ctx.debug_baumberg([tiny], [0], [ok], par)
    finally:
        tiny.free()


def test_debug_entry_is_the_production_path(ctx, modsx, oracle, small_pair):
    """modsx_detect_affine_keypoints (mode 0: no export cut, every converged keypoint is listed in detection order) against
    keypoints rebuilt from detect_scalespace and debug_baumberg(variant = 0, chunk = 0) on the pyramid's own blur levels, all
    octaves.  The levels come from the stage taps: the first level of octave 0 is gaussian_blur(image, sqrt(1.6^2 - 0.5^2)),
    octave_levels builds an octave's five levels from its first, and resize_half of level numberOfScales is the next octave's
    first level -- the chain of detectPyramidKeypoints (pyramid.cpp:455-573)."""
    img = small_pair[0]
    par = modsx.default_hessaff_params(mode=0, reg_number=1 << 20)
    im = ctx.upload(img)
    want = ctx.detect_affine_keypoints(im, par)
    ss = ctx.detect_scalespace(im, par)
    f32 = np.float32
    first = ctx.gaussian_blur(im, float(np.sqrt(f32(par.initialSigma) * f32(par.initialSigma) - f32(0.5) * f32(0.5))))
    im.free()
    min_size = 2 * par.border + 2
    planes, host, index, octave = [], [], {}, 0
    try:
        while first.shape[0] > min_size and first.shape[1] > min_size:
            fl = ctx.upload(first)
            blurs, _ = ctx.octave_levels(fl, par)
            fl.free()
            for level in range(1, par.numberOfScales + 1):        # detection levels 1 .. numberOfScales read the level below
                index[(octave, level)] = len(planes)
                planes.append(ctx.upload(blurs[level - 1]))
                host.append(blurs[level - 1])
            seed = ctx.upload(blurs[par.numberOfScales])
            first = ctx.resize_half(seed)
            seed.free()
            octave += 1
        assert octave >= 3 and set(ss["octave"].tolist()) <= set(range(octave)) and len(set(ss["octave"].tolist())) >= 2
        plane_of = np.array([index[(int(o), int(l))] for o, l in zip(ss["octave"], ss["level"])], np.int32)
        xyspd = np.stack([ss["x"], ss["y"], ss["s"], ss["pixelDistance"]], 1)
        got = ctx.debug_baumberg(planes, plane_of, xyspd, par)
    finally:
        for p in planes:
            p.free()
    assert got["geometry"] == modsx.baumberg_geometry(len(ss)) and got["geometry"]["kernel"] == 0
    assert (got["iters"] >= 0).all()
    keep = got["ok"] == 1
    assert 20 < keep.sum() < len(ss)
    rebuilt = np.zeros(int(keep.sum()), modsx.KEYPOINT)
    for f in ("x", "y", "s"):
        rebuilt[f] = ss[f][keep]
    for i, f in enumerate(("a11", "a12", "a21", "a22")):
        rebuilt[f] = got["u"][keep, i]
    rebuilt["response"] = ss["val"][keep]
    rebuilt["sub_type"] = ss["type"][keep]
    assert same_records(want, rebuilt)
    # and the oracle agrees on every keypoint of the list, failed ones included
    _compare(got, oracle.find_affine_shape_batch(host, plane_of, xyspd, oracle.default_params()), "production job list")
