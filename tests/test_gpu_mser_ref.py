"""GPU: the device MSER paths against the reference's OWN sources (oracle/_ref/libmser_ref.so through oracle.detect_msers_ref; only
oracle/_ref/ is read, never the reference's tree).  All comparisons are np.array_equal per field on the nine fields DetectMSERs
sets.

  * ctx.detect_msers (k_trunc_u8, download, the host tree) on f32 and on u8 uploads of the same pixels, at shapes around the front
    end's layout (a block is 8 rows of a view on one wavefront that walks a row 64 pixels at a time);
  * the planted TRUNC_VALUES images as f32: k_trunc_u8 judged by the reference's own (unsigned char)float, not by a model;
  * three non-identity views: ctx.synth_view -> ctx.detect_msers(view, tilt, zoom) against the reference on the downloaded pixels of
    that view -- the device chain synth -> trunc -> tree from the same pixels.

(1, 64): modsx_image_upload and modsx_image_wrap_device refuse images of fewer than 2 rows or columns (interpolate()'s clamp needs
two pixels per side), so no image handle of that shape exists for ctx.detect_msers.  The shape runs through the device front end
that does accept it -- ctx.debug_mser_front: k_trunc_u8 and the device bin sort -- and the host tree runs on the bytes the device
made; those keys are compared with the reference in the same way."""
import numpy as np
import pytest

import mser_front_cases as MC
import mser_ref_cases as RC
from common import need_mser_ref

pytestmark = pytest.mark.gpu

SHAPES = ((8, 64), (7, 63), (9, 65), (17, 129), (64, 96), (1, 64))
# the default set and the two budget sets keep min_size = 30 and max_area = 0.05, which leave no region in the shapes of a few hundred
# pixels; the last two are the same export cut with bounds those shapes can meet
PARAMS = (dict(), RC.LOOSE, RC.BUDGET_TILT, RC.BUDGET_ZOOM, dict(min_size=3, max_area=0.5, min_margin=3.0),
          dict(RC.BUDGET_TILT, min_size=3, max_area=0.5, reg_number=20))
PARAM_IDS = ("default", "loose", "budget_tilt3", "budget_zoom025", "small", "budget_small")


def _same(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for f in RC.FIELDS:
        assert np.array_equal(got[f], ref[f]), (what, f)


def _image(shape):
    """4 x 4-blocked noise: regions at every parameter set, also in the small shapes (integer grey values 0 .. 255)"""
    return RC.sweep_image("blocked", shape, 4000 + shape[0] * 131 + shape[1])


@pytest.fixture(scope="module")
def references(oracle):
    """the reference's answer per (shape, parameter set), computed once"""
    need_mser_ref(oracle)
    out = {}
    for shape in SHAPES:
        img = _image(shape)
        for pid, kw in zip(PARAM_IDS, PARAMS):
            k, tilt, zoom = RC.split_kw(kw)
            r = oracle.detect_msers_ref(img, tilt=tilt, zoom=zoom, **k)
            r.setflags(write=False)
            out[shape, pid] = r
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_uploads_against_the_reference(ctx, modsx, oracle, references, shape):
    need_mser_ref(oracle)
    img = _image(shape)
    total = 0
    if min(shape) < 2:
        with pytest.raises(RuntimeError):
            ctx.upload(img)
        u8 = ctx.debug_mser_front([img])[0][0]                     # the device's bytes of the one-row view
        assert u8.shape == shape
        for pid, kw in zip(PARAM_IDS, PARAMS):
            k, tilt, zoom = RC.split_kw(kw)
            _same(modsx.detect_msers_u8(u8, modsx.default_mser_params(**k), tilt=tilt, zoom=zoom), references[shape, pid], (shape, pid))
            total += len(references[shape, pid])
    else:
        for pixels in (img, img.astype(np.uint8)):
            im = ctx.upload(pixels)
            try:
                for pid, kw in zip(PARAM_IDS, PARAMS):
                    k, tilt, zoom = RC.split_kw(kw)
                    got = ctx.detect_msers(im, modsx.default_mser_params(**k), tilt=tilt, zoom=zoom)
                    _same(got, references[shape, pid], (shape, pid, pixels.dtype))
                    total += len(got)
            finally:
                im.free()
    assert total >= 20, (shape, total)                              # (1, 64) has 11 + 10 + 10 keys in the reference


def test_planted_values_against_the_references_conversion(ctx, modsx, oracle):
    """every value of TRUNC_VALUES (both zeros, negatives that wrap, values past the byte and past int32, infinities, NaN) in f32
    images through ctx.detect_msers: what k_trunc_u8 makes of them is what the reference's (unsigned char)*in_ptr makes of them"""
    need_mser_ref(oracle)
    cases = [(n, img, MC.MSER_LOOSE) for n, img in MC.trunc_cases().items()] + RC.trunc_block_cases()[::4]
    total = 0
    for name, img, kw in cases:
        ref = oracle.detect_msers_ref(img, **kw)
        im = ctx.upload(img)
        try:
            got = ctx.detect_msers(im, modsx.default_mser_params(**kw))
        finally:
            im.free()
        _same(got, ref, name)
        total += len(ref)
    assert total > 300


@pytest.mark.parametrize("tilt,phi,zoom", [(2.0, 0.0, 1.0), (2.5, 1.0, 1.0), (1.0, 0.0, 0.5)], ids=["tilt2", "tilt2.5_phi1", "zoom0.5"])
def test_synthesised_views_against_the_reference(ctx, modsx, oracle, tilt, phi, zoom):
    """synth_view -> detect_msers on the device's view against the reference on the same (downloaded) pixels"""
    need_mser_ref(oracle)
    from mods_amd import synthetic
    a = synthetic.blob_image(120, 160, 220, 11).astype(np.float32)
    kw = dict(min_size=10, max_area=0.2, min_margin=5.0)
    im = ctx.upload(a)
    view = None
    try:
        view, H, ident = ctx.synth_view(im, modsx.make_view(tilt, phi, zoom, 0.8, 1))
        assert not ident and (view.rows, view.cols) != a.shape
        pixels = view.download()
        assert pixels.size >= RC.MIN_PIXELS
        for k in (kw, dict(kw, mode=2, reg_number=60)):
            got = ctx.detect_msers(view, modsx.default_mser_params(**k), tilt=tilt, zoom=zoom)
            ref = oracle.detect_msers_ref(pixels, tilt=tilt, zoom=zoom, **k)
            _same(got, ref, (tilt, phi, zoom, k))
            assert len(ref) >= 20
    finally:
        if view is not None:
            view.free()
        im.free()
