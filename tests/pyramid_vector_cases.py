"""Inputs of the pyramid vector-tile suite and, restated in Python, the two rules its shapes are chosen against:

  - the tile fill of k_blur_hess<R, TH> loads the (TH + 4 + 2 R) x SW input tile in groups of four columns of a row pair; a group
    is VECTOR (one 16-byte load per row) iff its four columns lie inside the image, `0 <= gx0 and gx0 + 3 <= cols - 1`, and
    SCALAR (eight clamped loads) otherwise; rows are clamped one by one;
  - resize_half_px forms a destination pixel from a full 2 x 2 block, from the part of a block the source still has, or as 0;
    k_resize_half parks the resized values of a 64 x 8 tile and its one-pixel ring, the entries inside the destination only.

tests/test_pyramid_vector_cases_cpu.py proves from these rules what the shapes reach; tests/test_gpu_pyramid_vector_tiles.py
only compares with the oracle.  Images come from tests/pyramid_cases.image (fixed seeds).
"""
import numpy as np

from tests import pyramid_cases as PC

TW = 64                                  # tile width of k_blur_hess and k_resize_half
RESIZE_TH = 8                            # tile height of k_resize_half
HALF_WIDTHS = tuple(range(1, 9))         # R of PC.BLUR_SIGMAS, in its order

# ---- shapes ---------------------------------------------------------------------------------------------------------------------
BLUR_ROWS = (1, 3, 18, 35)
BLUR_COLS = (1, 3, 5, 8, 62, 67, 131, 197)
OCTAVE_SHAPES = ((35, 67), (18, 131), (33, 197), (17, 62))
PYRAMID_SHAPES = ((45, 67), (47, 133), (46, 131), (95, 259))


def uploadable(rows, cols):
    """the library takes images of at least 2 x 2 pixels (interpolate()'s clamp needs two per side); a shape with a side of one
    pixel stays in the lists and the GPU module requires its refusal"""
    return rows >= 2 and cols >= 2


def blur_image(R, rows, cols):
    return PC.image(rows, cols, 7000 + 1000 * R + 10 * rows + cols)


def octave_image(i):
    r, c = OCTAVE_SHAPES[i]
    return PC.image(r, c, 300 + i)


def pyramid_batch():
    return [PC.image(r, c, 400 + i) for i, (r, c) in enumerate(PYRAMID_SHAPES)]


# ---- the tile fill ----------------------------------------------------------------------------------------------------------------
def tile_dims(R, th):
    """(rows, needed columns, columns parked) of the input tile: TH + 4 + 2 R rows in pairs, 68 + 2 R columns rounded up to 4"""
    sh, sw = th + 4 + 2 * R, TW + 4 + 2 * R
    return sh, sw, (sw + 3) & ~3


def tile_origins(n, t):
    return list(range(0, n, t))


def is_vector(gx0, cols):
    return 0 <= gx0 and gx0 + 3 <= cols - 1


def fill_groups(R, cols, tx0):
    """[(first column, vector?)] of the groups of one tile row"""
    _, _, SW = tile_dims(R, 16)
    return [(gx0, is_vector(gx0, cols)) for gx0 in range(tx0 - 1 - R, tx0 - 1 - R + SW, 4)]


def fill_kind(R, cols, tx0):
    """'vector', 'scalar' or 'mixed': what the groups of a tile column are"""
    v = [x for _, x in fill_groups(R, cols, tx0)]
    return "vector" if all(v) else ("mixed" if any(v) else "scalar")


def pair_rows(R, th, rows, ty0):
    """[(image row of tile row 2 lp, of tile row 2 lp + 1)], each clamped on its own"""
    sh, _, _ = tile_dims(R, th)
    clamp = lambda y: min(max(y, 0), rows - 1)
    return [(clamp(ty0 - 1 - R + 2 * lp), clamp(ty0 - 1 - R + 2 * lp + 1)) for lp in range(sh // 2)]


def fill_tile(img, R, th, tx0, ty0):
    """the needed part of the input tile as the fill rule loads it: vector groups as slices of an image row, scalar groups column
    by clamped column"""
    rows, cols = img.shape
    sh, sw, SW = tile_dims(R, th)
    out = np.empty((sh, SW), np.float32)
    for lp, pair in enumerate(pair_rows(R, th, rows, ty0)):
        for k, gy in enumerate(pair):
            for g, (gx0, vec) in enumerate(fill_groups(R, cols, tx0)):
                if vec:
                    out[2 * lp + k, 4 * g:4 * g + 4] = img[gy, gx0:gx0 + 4]
                else:
                    out[2 * lp + k, 4 * g:4 * g + 4] = [img[gy, min(max(gx0 + q, 0), cols - 1)] for q in range(4)]
    return out[:, :sw]


def replicated_tile(img, R, th, tx0, ty0):
    """the same tile by definition: BORDER_REPLICATE around the image"""
    sh, sw, _ = tile_dims(R, th)
    y = np.clip(np.arange(ty0 - 1 - R, ty0 - 1 - R + sh), 0, img.shape[0] - 1)
    x = np.clip(np.arange(tx0 - 1 - R, tx0 - 1 - R + sw), 0, img.shape[1] - 1)
    return img[np.ix_(y, x)]


# ---- the resize -------------------------------------------------------------------------------------------------------------------
def half(n):
    """cvRound(n * 0.5): round half to even"""
    return int(round(n * 0.5))


def block_kind(sr, sc, dx, dy):
    """the branch of resize_half_px for destination pixel (dx, dy) of an sr x sc source"""
    if 2 * dy >= sr:
        return "zero"
    if 2 * dy + 2 <= sr and dx < sc // 2:
        return "full"
    return "zero" if 2 * dx >= sc else "partial"


def resize_by_rule(src):
    """the resized plane by the block rule, in f32 and in the kernel's order of additions"""
    sr, sc = src.shape
    out = np.zeros((half(sr), half(sc)), np.float32)
    for dy in range(out.shape[0]):
        for dx in range(out.shape[1]):
            kind = block_kind(sr, sc, dx, dy)
            if kind == "full":
                s = src[2 * dy:2 * dy + 2, 2 * dx:2 * dx + 2]
                out[dy, dx] = (np.float32(0) + (((s[0, 0] + s[0, 1]) + s[1, 0]) + s[1, 1])) * np.float32(0.25)
            elif kind == "partial":
                vals = src[2 * dy:2 * dy + 2, 2 * dx:2 * dx + 2].ravel()
                acc = np.float32(0)
                for v in vals:
                    acc = np.float32(acc + v)
                out[dy, dx] = acc / np.float32(len(vals))
    return out


def ring_entries(drows, dcols, tx0, ty0):
    """the (y, x) of a resize tile's ring (tile excluded) that lie inside the destination: the values it takes from its neighbours"""
    out = []
    for y in range(ty0 - 1, ty0 + RESIZE_TH + 1):
        for x in range(tx0 - 1, tx0 + TW + 1):
            inside_tile = ty0 <= y < ty0 + RESIZE_TH and tx0 <= x < tx0 + TW
            if not inside_tile and 0 <= y < drows and 0 <= x < dcols:
                out.append((y, x))
    return out
