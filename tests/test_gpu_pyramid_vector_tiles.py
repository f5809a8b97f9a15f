"""GPU: the 16-byte tile traffic of k_blur_hess (tile fill, store + Hessian) and the LDS-parked k_resize_half against the oracle,
on the shapes of tests/pyramid_vector_cases.py; tests/test_pyramid_vector_cases_cpu.py proves what those shapes reach.
Bar: bit-exact, through the entry points tests/test_gpu_pyramid.py uses; the launch counters must show the same launches.

  - gaussian_blur: every half width R = 1 .. 8 on 1 / 3 / 18 / 35 rows x 1 / 3 / 5 / 8 / 62 / 67 / 131 / 197 columns: tiles whose
    fill is all 16-byte loads, all scalar, or mixed on either edge; row pairs that clamp to one row; last tile columns of 62, 3
    and 5 pixels; planes whose rows start at every dword residue;
  - octave_levels: the fused Hessian and the four-pixel store on (35, 67), (18, 131), (33, 197), (17, 62);
  - debug_pyramids: a batch of (45, 67), (47, 133), (46, 131), (95, 259), every plane of every octave: the resize with a partial
    bottom row, a partial right column, two and three tile columns.
"""
import numpy as np
import pytest

from tests import pyramid_cases as PC
from tests import pyramid_vector_cases as VC

pytestmark = pytest.mark.gpu


def _moved(ctx, fn):
    before = ctx.detect_counters()
    out = fn()
    after = ctx.detect_counters()
    return out, {k: after[k] - before[k] for k in after}


def _launches(d):
    return {k: v for k, v in d.items() if v and not k.startswith("last_")}


def _zero_frame(resps):
    return not (resps[:, 0, :].any() or resps[:, -1, :].any() or resps[:, :, 0].any() or resps[:, :, -1].any())


@pytest.mark.parametrize("R", VC.HALF_WIDTHS)
def test_blur_every_half_width_on_vector_scalar_and_mixed_tiles(ctx, oracle, R):
    sigma = PC.BLUR_SIGMAS[R - 1]
    for rows in VC.BLUR_ROWS:
        for cols in VC.BLUR_COLS:
            img = VC.blur_image(R, rows, cols)
            if not VC.uploadable(rows, cols):          # one row or one column: refused before any launch
                before = ctx.detect_counters()
                with pytest.raises(RuntimeError, match="fewer than 2 rows or 2 columns"):
                    ctx.upload(img)
                assert ctx.detect_counters() == before
                continue
            im = ctx.upload(img)
            got, d = _moved(ctx, lambda: ctx.gaussian_blur(im, sigma))
            im.free()
            assert _launches(d) == {"blur_th16": 1, "blur_r%d" % R: 1}, (rows, cols, d)
            assert np.array_equal(got, oracle.gaussian_blur(img, sigma)), (rows, cols)


@pytest.mark.parametrize("i", range(len(VC.OCTAVE_SHAPES)), ids=["%dx%d" % s for s in VC.OCTAVE_SHAPES])
def test_octave_levels_fused_hessian_and_store(ctx, modsx, oracle, i):
    img = VC.octave_image(i)
    im = ctx.upload(img)
    (blurs, resps), d = _moved(ctx, lambda: ctx.octave_levels(im, modsx.default_hessaff_params()))
    im.free()
    assert _launches(d) == {"blur_th16": 4, "hessian": 1, "blur_r4": 1, "blur_r5": 1, "blur_r6": 1, "blur_r7": 1}
    rb, rr = oracle.octave_levels(img, oracle.default_params())
    assert np.array_equal(blurs, rb)
    assert np.array_equal(resps[:, 1:-1, 1:-1], rr[:, 1:-1, 1:-1])
    assert _zero_frame(resps)


def test_debug_pyramids_batch_every_plane(ctx, modsx, oracle):
    imgs = VC.pyramid_batch()
    ims = [ctx.upload(a) for a in imgs]
    p, po = modsx.default_hessaff_params(), oracle.default_params()
    got, d = _moved(ctx, lambda: ctx.debug_pyramids(ims, p))
    for im in ims:
        im.free()
    # octave 0: the first-level blur and four levels; octaves 1 and 2 (the last image only): a resize and four levels
    assert _launches(d) == {"blur_th16": 13, "resize": 2, "blur_r4": 3, "blur_r5": 4, "blur_r6": 3, "blur_r7": 3}
    L = p.numberOfScales + 2
    for i, img in enumerate(imgs):
        shapes = PC.octave_shapes(img.shape[0], img.shape[1], po.border)
        assert [b.shape[1:] for b, _ in got[i]] == shapes, i
        first = oracle.gaussian_blur(img, float(np.sqrt(np.float32(po.initialSigma) ** 2 - np.float32(0.25))))
        for o, (blurs, resps) in enumerate(got[i]):
            rb, rr = oracle.octave_levels(first, po, nlevels=L)
            assert np.array_equal(blurs, rb), (i, o)
            assert np.array_equal(resps[:, 1:-1, 1:-1], rr[:, 1:-1, 1:-1]), (i, o)
            assert _zero_frame(resps), (i, o)
            first = oracle.resize_half(rb[po.numberOfScales])
