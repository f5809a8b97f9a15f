"""GPU: the device directly against the reference's own code (oracle/_ref/libhessaff_ref.so: detectors/helpers.cpp,
matching/siftdesc.cpp and detectors/affinedetectors/affine.cpp compiled in place, oracle/ref_hessaff_shim.cpp), with no restatement
in between.  The reference side is computed on the host inside each test; oracle/_ref travels with the tree, the reference's
sources are not read here.

  SIFT       the planted patches of tests/sift_patch_cases.py, composed into its images, through Context.describe_regions (SIFT,
             RootSIFT, HalfSIFT, HalfRootSIFT), describe_regions_raw and extract_patches under photo_norm 0 and 1, against
             photometricallyNormalize + SIFTDescriptor on the same patches.  One image group per test.
  Baumberg   Context.debug_baumberg on baumberg_cases' jobs and Context.debug_affine_shape on affshape_cases' regions (each with
             ref_pin_cases' further jobs) against AffineShape::findAffineShape: the flag on every job, u as bits and iters where the
             reference converged.  The reference reports nothing else about a keypoint that did not converge.
  Sampling   Context.extract_patches on describe_cases' regions where DescribeRegions samples the image straight into the patch
             (the fast path, and the direct branch of the slow one) against interpolate.

Comparison rule: bit equality.  One exception, for f32 values that are NaN on both sides (the raw histogram of the overflow
patch): the sign and payload of a NaN are the processor's choice, not the reference's arithmetic.
"""
import numpy as np
import pytest

import describe_cases as DC
import ref_pin_cases as RC
import sift_patch_cases as SC
from common import need_hessaff_ref
from tests import affshape_cases as AC
from tests import baumberg_cases as BC

pytestmark = pytest.mark.gpu
F = np.float32


def same_or_both_nan(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


# ------------------------------------------------------------------------------------------------------------------------ SIFT
_REF = {}


def reference_of(oracle, im, q, pn):
    """dict(patch, raw f32, desc {type: f32 [128]}) of case q of image im from the reference, computed once: its interpolate on the
    composed image with the region's parameters (the identity harness of sift_patch_cases: the planted patch again, except that a
    planted -0 may come back as +0 -- 0 * d + v -- exactly as on the device), then photometricallyNormalize and SIFTDescriptor"""
    i = im["cases"][q]
    if ("sampled", i) not in _REF:
        cx, cy = (float(v) for v in im["centres"][q])
        sampled, touched = oracle.ref_interpolate(im["img"], cx, cy, 1.0, 0.0, 0.0, 1.0, SC.PS, SC.PS)
        assert not touched and np.array_equal(sampled, SC.planted()[i]["patch"])
        _REF[("sampled", i)] = sampled
    if (i, pn) not in _REF:
        p = _REF[("sampled", i)]
        patch = oracle.ref_photo_norm(p)[0] if pn else p
        desc, raw = {}, None
        for dt in range(4):
            desc[dt], raw = oracle.ref_sift(patch, dt)
        with np.errstate(all="ignore"):
            _REF[(i, pn)] = dict(patch=patch, raw=raw.astype(F), desc=desc)
    return _REF[(i, pn)]


@pytest.mark.parametrize("pn", [0, 1])
@pytest.mark.parametrize("group", ["+".join(g) for g in SC.GROUPS])
def test_sift_against_the_reference(ctx, modsx, oracle, group, pn):
    """every case of the group, every descriptor type, under this photo_norm -- also the families that
    tests/test_gpu_sift_patches.py runs under photo_norm 0 alone"""
    need_hessaff_ref(oracle)
    ims = [im for im in SC.images() if im["group"] == group]
    assert len(ims) == dict(zip(("+".join(g) for g in SC.GROUPS), SC.IMAGES_PER_GROUP))[group]
    total = 0
    for im in ims:
        handle = ctx.upload(im["img"])
        try:
            regs = SC.regions(modsx.REGION, im["centres"])
            refs = [reference_of(oracle, im, q, pn) for q in range(len(im["cases"]))]
            names = [SC.planted()[i]["name"] for i in im["cases"]]
            kw = dict(mr_size=SC.MR_SIZE, fast=SC.FAST, photo_norm=pn)
            got = ctx.extract_patches(handle, regs, **kw)
            for q, r in enumerate(refs):
                assert same_or_both_nan(got[q], r["patch"]), (names[q], pn, "patch")
            got = ctx.describe_regions_raw(handle, regs, **kw)
            for q, r in enumerate(refs):
                assert same_or_both_nan(got[q], r["raw"]), (names[q], pn, "raw histogram", np.nonzero(got[q] != r["raw"])[0][:8])
            for dt in range(4):
                got = ctx.describe_regions(handle, regs, desc_type=dt, **kw)
                for q, r in enumerate(refs):
                    assert np.array_equal(got[q], r["desc"][dt]), (names[q], pn, dt, np.nonzero(got[q] != r["desc"][dt])[0][:8])
            total += len(refs)
        finally:
            handle.free()
    assert total == sum(SC.family_counts()[f] for f in group.split("+"))


# -------------------------------------------------------------------------------------------------------------------- Baumberg
def _compare_shapes(got, ref, what):
    """got: the device's u / ok / iters per job; ref: the reference's hit / u / iters"""
    n = len(ref["hit"])
    assert len(got["ok"]) == n, what
    assert np.array_equal(got["ok"], ref["hit"]), (what, "flag", np.nonzero(got["ok"] != ref["hit"])[0][:10])
    h = ref["hit"] == 1
    gu, ru = np.ascontiguousarray(got["u"], F).view(np.uint32), ref["u"].view(np.uint32)
    assert np.array_equal(gu[h], ru[h]), (what, "u", np.nonzero((gu != ru).any(1) & h)[0][:10])
    assert np.array_equal(got["iters"][h], ref["iters"][h]), (what, "iters")
    return h


@pytest.mark.parametrize("variant", [0, 3])
def test_baumberg_against_the_reference(ctx, modsx, oracle, variant):
    need_hessaff_ref(oracle)
    po, xy = RC.baumberg_jobs()
    planes = BC.planes(oracle)
    ref = oracle.ref_find_affine_shape_batch(planes, po, xy, oracle.default_params())
    dplanes = [ctx.upload(p) for p in planes]
    try:
        got = ctx.debug_baumberg(dplanes, po, xy, modsx.default_hessaff_params(), variant=variant)
    finally:
        for im in dplanes:
            im.free()
    assert got["geometry"]["kernel"] == variant
    h = _compare_shapes(got, ref, "variant %d" % variant)
    assert all(4 * int(h[po == p].sum()) >= int((po == p).sum()) for p in range(len(planes)))


@pytest.mark.parametrize("W", [5, 11, 17])
def test_baumberg_other_windows_against_the_reference(ctx, modsx, oracle, W):
    need_hessaff_ref(oracle)
    po, xy = BC.subset(300)
    planes = BC.planes(oracle)
    ref = oracle.ref_find_affine_shape_batch(planes, po, xy, oracle.default_params(smmWindowSize=W))
    dplanes = [ctx.upload(p) for p in planes]
    try:
        got = ctx.debug_baumberg(dplanes, po, xy, modsx.default_hessaff_params(smmWindowSize=W))
    finally:
        for im in dplanes:
            im.free()
    assert _compare_shapes(got, ref, "W %d" % W).sum() >= 10          # at W = 3 the reference converges on none of them


def test_affine_shape_against_the_reference(ctx, modsx, oracle):
    need_hessaff_ref(oracle)
    imgs, lists = AC.images(oracle), RC.affshape_lists()
    refs = [RC.reference_affshape(oracle, img, regs) for img, regs in zip(imgs, lists)]
    dimgs = [ctx.upload(p) for p in imgs]
    try:
        got = ctx.debug_affine_shape(dimgs, lists)
    finally:
        for im in dimgs:
            im.free()
    border = np.concatenate([r["border"] for r in refs])
    assert np.array_equal(got["border"], border) and got["launched"] == int((~border).sum())
    run = ~border
    ref = {f: np.concatenate([r[f] for r in refs])[run] for f in ("hit", "u", "iters")}
    h = _compare_shapes({f: got[f][run] for f in ("ok", "u", "iters")}, ref, "debug_affine_shape")
    assert h.sum() >= 200 and (~h).sum() >= 100


# ----------------------------------------------------------------------------------------------------------------- patch sampling
@pytest.mark.parametrize("pn", [0, 1])
def test_patch_sampling_against_the_reference(ctx, modsx, oracle, pn):
    need_hessaff_ref(oracle)
    img = DC.image()
    regs = np.concatenate([DC.regions_of(P) for P in DC.SIZES + (0,)] + [DC.crafted_regions()[::7]])
    handle = ctx.upload(img)
    try:
        seen = set()
        for fast in (1, 0):
            calls = [RC.sampling_call(k, DC.MR_SIZE, fast=bool(fast)) for k in regs["det_kp"]]
            sel = np.array([q for q, c in enumerate(calls) if c is not None])
            assert len(sel) == len(regs) if fast else 6 <= len(sel) < len(regs)
            got = ctx.extract_patches(handle, regs[sel], mr_size=DC.MR_SIZE, fast=fast, photo_norm=pn)
            for row, q in enumerate(sel):
                want, touched = oracle.ref_interpolate(img, *calls[q], 41, 41)
                if pn:
                    want = oracle.ref_photo_norm(want)[0]
                assert same_or_both_nan(got[row], want), ("fast" if fast else "direct", int(q), float(regs["det_kp"]["s"][q]))
                seen.add((fast, touched))
        assert seen == {(f, t) for f in (0, 1) for t in (False, True)}      # both of interpolate's branches, both return values
    finally:
        handle.free()
