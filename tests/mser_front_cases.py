"""Models and cases of the MSER front end on the device (k_trunc_u8, k_mser_hist / _scan / _scatter, the block layout of
mser_front in engine_views.hip) and of the grey ingest (k_gray_u8 / k_gray_f32), in plain numpy.

The models restate the operations, not the kernels:
  trunc_u8_model   (unsigned char)float as x86 evaluates it (cvttss2si, low byte), DetectMSERs' `*ptr = (unsigned char)*in_ptr`
                   (extrema.cpp:401-403) and the oracle's oracle_mser.cpp:348; tests/test_mser_front_cases_cpu.py pins it to the
                   oracle as built, and tests/test_mser_ref_cpu.py to that very line of the reference as built (the reference on
                   f32 pixels == the reference on this model's bytes, at every planted value)
  bin_sort_model   the stable counting sort by grey level that the component tree walks (sortPixels.cpp:76-125): 257 level starts
                   and the pixels' padded offsets (r + 1) * (cols + 2) + c + 1
  gray_model       the 3-channel ingest, f32(f64(f32(B + G)) * k + f64(R) * k) with the f64 constant k = 1. / 3.0
The cases are the smallest shapes that reach each path of the sort: a block is MSB_ROWS = 8 rows of one view on one wavefront that
walks a row 64 pixels at a time; a launch set holds up to MAXB = 32 views."""
import numpy as np

from mods_amd import synthetic

MSB_ROWS, WAVE, MAXB = 8, 64, 32

# what trunc_cases() plants: zeros of both signs, fractions that truncate toward zero, negatives that wrap, the byte's ends, values
# past the byte, the last f32 below 2^31, 2^31 itself, -2^31 (the last value in range), the first f32 below it, and everything
# outside int32
TRUNC_VALUES = np.array([-0.0, -0.5, -0.99, -1, -1.5, -255, -256, -300, 255, 255.99, 256, 300, 511.9, 65536, 2147483520, 2.0 ** 31,
                         -2.0 ** 31, -2147483904, 2.0 ** 32, 1e30, -1e30, np.inf, -np.inf, np.nan], np.float32)


def trunc_u8_model(f32):
    """(unsigned char)v as x86 compiles it: cvttss2si truncates toward zero into int32 and the low byte is kept; values outside
    [-2^31, 2^31), NaN and both infinities convert to the `integer indefinite` 0x80000000, whose low byte is 0."""
    v = np.asarray(f32, np.float32)
    ok = np.isfinite(v) & (v >= np.float32(-2.0 ** 31)) & (v < np.float32(2.0 ** 31))
    t = np.trunc(np.where(ok, v, np.float32(0)).astype(np.float64)).astype(np.int64)     # exact: every f32 in range is an f64
    return np.where(ok, t & 255, 0).astype(np.uint8)


def bin_sort_model(u8):
    """(start [257] int32, order [rows * cols] int32) of a 2-d u8 image: start[l] = pixels below level l, start[256] = all;
    order = the pixels by (grey level, raster position) as padded offsets (r + 1) * (cols + 2) + c + 1."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 2
    rows, cols = u8.shape
    flat = u8.ravel()
    start = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=256))]).astype(np.int32)
    idx = np.argsort(flat, kind="stable")
    r, c = idx // cols, idx % cols
    return start, ((r + 1) * (cols + 2) + c + 1).astype(np.int32)


def gray_model(pixels):
    """[rows, cols, 3] u8 or f32 (B, G, R) -> f32 grey as k_gray_u8 / k_gray_f32 state it: t = f32(B + G) in f32, then
    f32(f64(t) * k + f64(R) * k), k = 1. / 3.0 in f64 (two roundings of the products, one of the sum, one to f32)."""
    p = np.asarray(pixels)
    assert p.ndim == 3 and p.shape[2] == 3
    p = p.astype(np.float32)
    k = np.float64(1.0) / np.float64(3.0)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (p[..., 0] + p[..., 1]).astype(np.float32)
        return (t.astype(np.float64) * k + p[..., 2].astype(np.float64) * k).astype(np.float32)


def sort_cases():
    """name -> u8 image"""
    rs = np.random.RandomState(20240)
    out = {}
    for r, c in ((1, 1), (1, 37), (23, 1), (2, 2), (8, 64), (7, 63), (9, 65), (16, 128), (17, 129), (8, 200)):
        out["random_%dx%d" % (r, c)] = rs.randint(0, 256, (r, c)).astype(np.uint8)
    out["constant77_40x50"] = np.full((40, 50), 77, np.uint8)                                # one value in every lane of every step
    out["columns_16x256"] = np.tile(np.arange(256, dtype=np.uint8), (16, 1))                 # 64 different values in every step
    out["rows_24x70"] = np.tile(np.arange(24, dtype=np.uint8)[:, None] * 10, (1, 70))        # one value per row, three blocks
    yy, xx = np.mgrid[:16, :130]
    out["checker_0_255_16x130"] = (((yy + xx) & 1) * 255).astype(np.uint8)                   # the end buckets, 32 lanes per value
    out["three_levels_33x100"] = np.array([3, 128, 250], np.uint8)[rs.randint(0, 3, (33, 100))]
    out["uniform_64x96"] = rs.randint(0, 256, (64, 96)).astype(np.uint8)
    out["no_0_no_255_20x90"] = rs.randint(1, 255, (20, 90)).astype(np.uint8)                 # buckets 0 and 255 empty
    return out


def batch_cases():
    """name -> list of u8 views of one launch set"""
    s = sort_cases()
    names = list(s)
    big = [n for n in names if s[n].shape[0] >= MSB_ROWS and s[n].size > 1]
    full = [s[big[i % len(big)]] for i in range(MAXB)]
    full[MAXB // 2] = s["random_7x63"]          # rows < MSB_ROWS in the middle: one short block between full ones
    full[5] = s["random_1x37"]
    full[20] = s["random_23x1"]
    full[MAXB - 1] = s["random_1x1"]            # a one-pixel view last: the last block, the last place of `order`
    assert len(full) == MAXB
    return {"maxb_mixed": full, "large_then_small": [s["uniform_64x96"], s["random_2x2"]]}


def _plant(img, values, rs):
    """values at scattered places of the float4 body, and -- rotating through the list -- in the last n % 4 pixels (the scalar tail)"""
    out = np.ascontiguousarray(img, np.float32).copy()
    flat = out.reshape(-1)
    n = flat.size
    body = n - n % 4
    at = rs.choice(body, 4 * len(values), replace=False)
    flat[at] = np.tile(values, 4)                # every value in several lanes of the 4-pixel group
    for k in range(n % 4):
        flat[body + k] = values[(7 * (n % 4) + k) % len(values)]
    return out


def trunc_cases():
    """name -> f32 blob image (it yields MSER regions) with TRUNC_VALUES planted, at pixel counts n % 4 = 0, 1, 2, 3"""
    rs = np.random.RandomState(77)
    out = {}
    for rows, cols in ((96, 128), (95, 127), (97, 126), (97, 127)):
        assert (rows * cols) % 4 == len(out)
        img = synthetic.blob_image(rows, cols, 150, 401).astype(np.float32)
        out["blobs_%dx%d_rem%d" % (rows, cols, (rows * cols) % 4)] = _plant(img, TRUNC_VALUES, rs)
    return out


MSER_MID = dict(min_size=10, max_area=0.2, min_margin=5.0)
MSER_LOOSE = dict(min_size=1, min_margin=2.0, max_area=1.0)      # the loose set of tests/test_mser_cpu.py


def engine_cases():
    """name -> dict(image f32, scales, tilts, phi, sigma, mser): view sets for detect_describe_views with the MSER detector, at
    the edges of the front end.  The view list is set_vs_pars(scales, tilts, phi, sigma, 1).
      steps_scales / ramp_scales   the step and the ramp image of tests/test_mser_cpu.py at scales 1, 0.25, 0.125: views of 22 x 31 and
                      11 x 15 pixels in one set with the full-size view
      trunc_identity  a blob image with the planted values of up to 2^32 in magnitude, identity view.  (+-1e30, the infinities and NaN
                      stay out of THIS image: a patch that holds them has overflowing or NaN gradients, and the oracle's
                      orientation stage -- like the reference's -- then indexes its angle table with (int) of a NaN and crashes.
                      trunc_cases() carries the whole list for the stages that are defined on it.)
      blob_61_views / blob_51_views   more than MAXB views of a 64 x 80 blob image (tilts 1, 2, 4, 6, 8 at phi 60 / phi 72): two
                      launch sets, the second with another layout in the same buffers"""
    from test_mser_cpu import _images
    im = _images()
    ramp, steps = im[4], im[5]
    assert ramp.shape == (100, 140) and steps.shape == (90, 130)
    v = TRUNC_VALUES[np.isfinite(TRUNC_VALUES) & (np.abs(TRUNC_VALUES) <= np.float32(2.0 ** 32))]
    planted = _plant(synthetic.blob_image(95, 127, 150, 401).astype(np.float32), v, np.random.RandomState(77))
    blob = synthetic.blob_image(64, 80, 60, 402).astype(np.float32)
    zooms = dict(scales=[1.0, 0.25, 0.125], tilts=[1.0], phi=360.0, sigma=0.8, mser=MSER_LOOSE)
    return {"steps_scales": dict(image=steps, **zooms), "ramp_scales": dict(image=ramp, **zooms),
            "trunc_identity": dict(image=planted, scales=[1.0], tilts=[1.0], phi=360.0, sigma=0.8, mser=MSER_MID),
            "blob_61_views": dict(image=blob, scales=[1.0], tilts=[1, 2, 4, 6, 8], phi=60.0, sigma=0.8, mser=MSER_MID),
            "blob_51_views": dict(image=blob, scales=[1.0], tilts=[1, 2, 4, 6, 8], phi=72.0, sigma=0.8, mser=MSER_MID)}


def trunc_strips():
    """f32 views 1 x L of TRUNC_VALUES: L = 1, 2, 3 (the kernel's scalar tail only, every value at every tail place), L = 24 (the
    float4 body only) and L = 5, 6, 7 (one float4 and a tail).  They give no regions: for the truncation alone."""
    v = TRUNC_VALUES
    out = [v.reshape(1, -1).copy()]
    for L in (1, 2, 3):
        for s in range(len(v)):
            out.append(np.roll(v, -s)[:L].reshape(1, L).copy())
    for L in (5, 6, 7):
        for s in range(0, len(v), 4):
            out.append(np.roll(v, -s)[:L].reshape(1, L).copy())
    return out
