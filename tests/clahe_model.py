"""numpy restatement of cv::CLAHE::apply -- CLAHE_Impl::apply of OpenCV 2.4.9 (modules/imgproc/src/clahe.cpp), variant 0, and
the rule of OpenCV 3.x / 4.x, variant 1 -- stage by stage: source bytes, geometry, LUT source, histograms, LUTs, output.

Written from the contract text of include/modsx.h alone and independent of the C++: it makes the padded copy the library
never makes, reflects by the iterative borderInterpolate rule, and loops over tiles.  Every f32 operation is one numpy
operation on float32 arrays, so nothing is contracted; np.rint rounds half to even as the conversions of the contract do.
tiles = (tiles_x, tiles_y), as cv::Size(width, height)."""
import numpy as np

H = 256


def to_u8(img):
    """saturate_cast<uchar> of the gray f32 values: round to nearest even, clamp to 0..255, NaN -> 0"""
    f = np.asarray(img, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint(f)
        r = np.where(np.isnan(r), np.float32(0), r)
        return np.clip(r, 0, 255).astype(np.uint8)


def reflect101(p, n):
    """borderInterpolate(p, n, BORDER_REFLECT_101)"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def geometry(rows, cols, clip=4.0, tiles=(8, 8)):
    tx, ty = tiles
    if cols % tx == 0 and rows % ty == 0:
        pad_rows, pad_cols = rows, cols
    else:
        pad_rows, pad_cols = rows + (ty - rows % ty), cols + (tx - cols % tx)
    tile_w, tile_h = pad_cols // tx, pad_rows // ty
    total = tile_w * tile_h
    lut_scale = np.float32(H - 1) / np.float32(total)
    clip_limit = max(int(float(clip) * total / H), 1) if clip > 0 else 0
    return dict(tile_w=tile_w, tile_h=tile_h, pad_cols=pad_cols, pad_rows=pad_rows, clip_limit=clip_limit, lut_scale=np.float32(lut_scale))


def lut_source(u8, geo):
    rows, cols = u8.shape
    yy = [reflect101(y, rows) for y in range(geo["pad_rows"])]
    xx = [reflect101(x, cols) for x in range(geo["pad_cols"])]
    return u8[np.ix_(yy, xx)]


def histograms(src, geo, tiles):
    tx, ty = tiles
    tw, th = geo["tile_w"], geo["tile_h"]
    hist = np.zeros((tx * ty, H), np.int64)
    for tyi in range(ty):
        for txi in range(tx):
            roi = src[tyi * th:(tyi + 1) * th, txi * tw:(txi + 1) * tw]
            hist[tyi * tx + txi] = np.bincount(roi.ravel(), minlength=H)
    return hist


def luts(hist, geo, variant=0):
    """-> (lut [tiles][256] u8, clipped [tiles], residual [tiles]) (the latter two zero without clipping)"""
    clip_limit, scale = geo["clip_limit"], geo["lut_scale"]
    nt = len(hist)
    lut = np.zeros((nt, H), np.uint8)
    clipped_all, residual_all = np.zeros(nt, np.int64), np.zeros(nt, np.int64)
    for k in range(nt):
        h = hist[k].copy()
        if clip_limit > 0:
            clipped = int(np.maximum(h - clip_limit, 0).sum())
            h = np.minimum(h, clip_limit)
            batch = clipped // H
            residual = clipped - batch * H
            clipped_all[k], residual_all[k] = clipped, residual
            h += batch
            if variant == 0:
                h[:residual] += 1
            elif residual:
                step = max(H // residual, 1)
                i = 0
                while i < H and residual > 0:
                    h[i] += 1
                    i += step
                    residual -= 1
        s = np.cumsum(h).astype(np.float32) * scale
        lut[k] = to_u8(s)
    return lut, clipped_all, residual_all


def axis_terms(n, tile, ntiles, variant=0):
    """(t1, t2, a) of the coordinates 0 .. n - 1 along one axis"""
    i = np.arange(n, dtype=np.float32)
    if variant == 0:
        f = i / np.float32(tile) - np.float32(0.5)
    else:
        f = i * (np.float32(1.0) / np.float32(tile)) - np.float32(0.5)
    fl = np.floor(f)
    a = (f - fl).astype(np.float32)
    t1 = fl.astype(np.int64)
    t2 = np.minimum(t1 + 1, ntiles - 1)
    t1 = np.maximum(t1, 0)
    return t1, t2, a


def interpolate(l11, l12, l21, l22, xa, ya, variant=0):
    """res (f32) of the four LUT values (f32 arrays) and the weights"""
    one = np.float32(1.0)
    if variant == 0:
        res = np.zeros_like(l11, dtype=np.float32)
        res = res + l11 * ((one - xa) * (one - ya))
        res = res + l12 * (xa * (one - ya))
        res = res + l21 * ((one - xa) * ya)
        res = res + l22 * (xa * ya)
        return res
    xa1, ya1 = one - xa, one - ya
    return (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya


def apply_luts(u8, lut, geo, tiles, variant=0, formula=None):
    """-> (out u8, res f32); formula: the interpolation variant when it is to differ from the coordinate variant"""
    tx, ty = tiles
    rows, cols = u8.shape
    ty1, ty2, ya = axis_terms(rows, geo["tile_h"], ty, variant)
    tx1, tx2, xa = axis_terms(cols, geo["tile_w"], tx, variant)
    ya, xa = ya[:, None], xa[None, :]
    v = u8.astype(np.int64)
    f = lambda a, b: lut[a[:, None] * tx + b[None, :], v].astype(np.float32)      # noqa: E731
    res = interpolate(f(ty1, tx1), f(ty1, tx2), f(ty2, tx1), f(ty2, tx2), np.broadcast_to(xa, u8.shape), np.broadcast_to(ya, u8.shape),
                      variant if formula is None else formula)
    return to_u8(res), res


def run(img, clip=4.0, tiles=(8, 8), variant=0):
    """every stage for one gray f32 (or u8) image -> dict(u8, geo, hist, lut, clipped, residual, out, res)"""
    u8 = to_u8(img)
    geo = geometry(u8.shape[0], u8.shape[1], clip, tiles)
    hist = histograms(lut_source(u8, geo), geo, tiles)
    lut, clipped, residual = luts(hist, geo, variant)
    out, res = apply_luts(u8, lut, geo, tiles, variant)
    return dict(u8=u8, geo=geo, hist=hist, lut=lut, clipped=clipped, residual=residual, out=out, res=res)
