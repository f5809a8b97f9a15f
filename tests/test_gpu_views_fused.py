"""GPU: the one-launch view synthesis (rotate + blur at the tapped columns / rows + tilt, k_views_fused) against the oracle.

Every comparison is np.array_equal with oracle.synth_view: same operations on the same operands in the same order, only fewer
of them.  The last test keeps the others from passing on the separate launches alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEADLINE = ([1.0], [1, 2, 4, 6, 8], 120.0, 0.2, 1)     # the 31 views bench.py measures


def _noise_u8(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def _check_view(ctx, oracle, modsx, im, ref_pixels, view_args):
    vo, vm = oracle.make_view(*view_args), modsx.make_view(*view_args)
    ref, Href, ident_ref = oracle.synth_view(ref_pixels, vo)
    got, H, ident = ctx.synth_view(im, vm)
    try:
        assert ident == ident_ref and np.array_equal(H, Href), view_args
        assert (got.rows, got.cols) == ref.shape, view_args
        out = got.download()
        assert np.array_equal(out, ref), (view_args, int((out != ref).sum()), np.argwhere(out != ref)[:4].tolist())
    finally:
        got.free()


@pytest.mark.parametrize("rows,cols", [(768, 1024), (479, 641)])
def test_headline_views_bit_exact_u8_and_f32(ctx, modsx, oracle, rows, cols):
    """All 30 non-identity views of the headline view set, from a u8 upload and from an f32 upload of the same pixels."""
    a = _noise_u8(rows, cols, 5)
    vo = oracle.set_vs_pars(*HEADLINE, [])
    vm = modsx.set_vs_pars(*HEADLINE, [])
    assert len(vo) == len(vm) == 31
    refs = [oracle.synth_view(a.astype(np.float32), v) for v in vo]
    assert sum(1 for _, _, ident in refs if not ident) == 30
    for pixels in (a, a.astype(np.float32)):
        im = ctx.upload(pixels)
        for v, (ref, Href, ident_ref) in zip(vm, refs):
            got, H, ident = ctx.synth_view(im, v)
            assert ident == ident_ref and np.array_equal(H, Href)
            if not ident:
                out = got.download()
                assert out.shape == ref.shape
                assert np.array_equal(out, ref), (pixels.dtype, v.tilt, v.phi, int((out != ref).sum()), np.argwhere(out != ref)[:4].tolist())
            got.free()
        im.free()


@pytest.mark.parametrize("tilt,phi,zoom,sigma", [
    # non-integer tilts: 1/32-pixel fractions in x, all of a row's two taps carry weight
    (2.5, 0.7, 1.0, 0.2), (3.3, 2.0, 1.0, 0.5), (1.5, 0.4, 1.0, 0.5), (7.7, 2.9, 1.0, 0.2),
    # zoomed views: fractions in x and y, all four taps carry weight; rows are tapped sparsely too
    (3.0, 0.4, 0.5, 0.5), (1.0, 0.0, 0.25, 0.5), (1.0, 0.0, 0.125, 0.8), (2.0, 1.9, 0.7, 0.2), (6.0, 0.3, 0.25, 0.8),
    # wider filters inside the fused kernel's halo
    (8.0, 1.0, 1.0, 1.0), (4.0, 2.5, 1.0, 1.5), (9.0, 0.0, 1.0, 0.8)])
@pytest.mark.parametrize("rows,cols", [(300, 421), (768, 1024)])
def test_fractional_tilts_and_zooms_bit_exact(ctx, modsx, oracle, rows, cols, tilt, phi, zoom, sigma):
    a = _noise_u8(rows, cols, 11)
    im = ctx.upload(a)
    try:
        _check_view(ctx, oracle, modsx, im, a.astype(np.float32), (tilt, phi, zoom, sigma, 1))
    finally:
        im.free()


SMALL_VIEWS = ((2.0, 0.0, 1.0, 0.2, 1), (2.0, 1.1, 1.0, 0.5, 1), (2.5, 0.3, 1.0, 0.5, 1), (1.0, 0.0, 0.5, 0.5, 1))   # >= 1 output pixel of a 3 x 3 image
MORE_VIEWS = ((8.0, 2.0, 1.0, 0.2, 1), (4.0, np.pi / 2, 1.0, 0.2, 1), (3.0, 2.6, 0.5, 0.5, 1))                     # need >= 15 pixels per side


@pytest.mark.parametrize("rows,cols", [(3, 3), (3, 200), (200, 3), (5, 7), (16, 128), (17, 129), (15, 127), (130, 18), (33, 257)])
def test_images_smaller_than_a_tile_bit_exact(ctx, modsx, oracle, rows, cols):
    """Images narrower and lower than one VF_TW x VF_TH tile, and just around its size: the +1 tap column / row, the halo's
    reflection and the ownership of pixels whose taps leave the rotated image."""
    a = _noise_u8(rows, cols, 23)
    im = ctx.upload(a)
    try:
        for args in SMALL_VIEWS + (MORE_VIEWS if min(rows, cols) >= 15 else ()):
            _check_view(ctx, oracle, modsx, im, a.astype(np.float32), args)
    finally:
        im.free()


def test_f32_image_with_negative_values_and_minus_zero(ctx, modsx, oracle):
    """An f32 upload need not be non-negative: negative pixels, -0.0, pixels of large magnitude and both signs.  With tap
    fractions of exactly 0 (integer tilts) the products with the zero weights still enter the sum as the oracle forms it."""
    rng = np.random.default_rng(31)
    a = (rng.standard_normal((240, 333)) * 300.0).astype(np.float32)
    a[::7, ::5] = -0.0
    a[3::11, 2::13] = 0.0
    a[5::17, 1::19] = -1e30
    a[8::23, 4::29] = 1e30
    a[100:120, 50:90] = -255.0
    im = ctx.upload(a)
    try:
        for args in ((2.0, 0.0, 1.0, 0.2, 1), (4.0, 0.8, 1.0, 0.2, 1), (8.0, 2.2, 1.0, 0.2, 1), (6.0, 1.5, 1.0, 0.5, 1),
                     (2.5, 0.7, 1.0, 0.2, 1), (3.0, 0.4, 0.5, 0.5, 1)):
            _check_view(ctx, oracle, modsx, im, a, args)
    finally:
        im.free()


def test_headline_view_set_takes_the_fused_kernel_only(modsx):
    """All 30 non-identity views of the headline view set go through the one-launch kernel: no launch of the separate
    rotate / tilt warps is left.  A context of its own: profiling taxes a context for good."""
    from mods_amd import synthetic
    a, _, _ = synthetic.make_pair(rows=768, cols=1024, nblobs=4000, seed=12345)
    views = modsx.set_vs_pars(*HEADLINE, [])
    assert len(views) == 31
    c = modsx.Context(0)
    try:
        c.profile(True)
        im = c.upload(a)
        regs, _ = c.detect_describe_views(im, views, modsx.default_pair_params(), want_desc=False)
        st = c.kernel_stats()
        im.free()
        assert len(regs) > 10000
        assert st["warp_affine"]["launches"] == 0, st["warp_affine"]
        assert st["view_blur"]["launches"] >= 1, st["view_blur"]
    finally:
        c.close()
