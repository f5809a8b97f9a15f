"""Cases of the MSER comparison with the reference's own sources (oracle/_ref/libmser_ref.so, oracle.detect_msers_ref): plain numpy
on fixed RandomState seeds.  A case is (name, f32 image, keywords of detect_msers / detect_msers_ref, tilt and zoom among them).

What the reference cannot be handed, and so is not here:
  * images under 64 pixels -- it faults on tiny images (every one tried under 30 pixels; 64 is a margin, oracle/pyoracle.py);
  * a region that is stable at threshold 0: RegionBoundaries (boundary.cpp:149-189) marks the pixels of a component with
    `marker = thresh` in a picture that memset cleared to 0, so at threshold 0 nothing is ever marked, the region's RLE stays empty,
    RLE2Ellipse divides by an area of 0 and Matrix2::schur_sym (utls/matrix.cpp:188-193) ends the PROCESS with exit(-1) on the NaN
    covariance.  thresh = pos + margin / 2 is 0 only for pos = 0 and margin <= 1, and a margin has to exceed min_margin, so every
    case here with a FIXED_TH min_margin >= 1 (the other export modes detect at 1.0) is safe by construction; the cases with
    relative = 1 or min_margin < 1 were each run once in a child process before they were listed.  The product and the restatement
    return a key for such a region; the reference's own program would have ended there.
A stable threshold of 255, which mser.cpp and oracle_mser.cpp skip, cannot occur for min_margin >= 0: pos + margin <= 255 and
thresh = pos + margin / 2 leave pos = 255, margin = 0, whose quality 0 (0 / 0 in relative mode) never exceeds min_margin.  The highest
one, 254, is planted below.
(64, 1): one-column images of 64 and more pixels run in the reference (checked in a child process first) and are in the sweep."""
import numpy as np

from mser_front_cases import TRUNC_VALUES
from test_mser_cpu import PARAM_SETS, _images

FIELDS = ("x", "y", "a11", "a12", "a21", "a22", "s", "response", "sub_type")     # the nine fields DetectMSERs sets
MIN_PIXELS = 64

LOOSE = dict(min_size=1, min_margin=1.0, max_area=1.0)
HALF_RELATIVE = dict(min_size=2, min_margin=1.0, max_area=0.5, relative=1)
BUDGET_TILT = dict(mode=2, reg_number=60, tilt=3.0)
BUDGET_ZOOM = dict(mode=2, reg_number=60, zoom=0.25)
PROMOTE = dict(min_size=12000, max_area=1.0, min_margin=2.0)     # promoteAt = min(10000, min_size) < min_size: 130 x 130 only
SWEEP_PARAMS = list(PARAM_SETS) + [LOOSE, HALF_RELATIVE, BUDGET_TILT, BUDGET_ZOOM]
SWEEP_SHAPES = ((64, 64), (65, 63), (33, 200), (200, 33), (17, 19), (8, 8), (2, 50), (50, 2), (1, 64), (64, 1), (130, 130))
SWEEP_KINDS = ("noise", "four_levels", "blocked", "wave", "binary", "nested")


def sweep_image(kind, shape, seed):
    rs = np.random.RandomState(seed)
    rows, cols = shape
    if kind == "noise":
        return rs.randint(0, 256, shape).astype(np.float32)
    if kind == "four_levels":                                  # large plateaus and ties: levels 0, 80, 160, 240
        return (rs.randint(0, 4, shape) * 80).astype(np.float32)
    if kind == "blocked":                                      # 4 x 4 blocks of one random level
        b = rs.randint(0, 256, ((rows + 3) // 4, (cols + 3) // 4))
        return np.kron(b, np.ones((4, 4), int))[:rows, :cols].astype(np.float32)
    if kind == "wave":
        yy, xx = np.mgrid[:rows, :cols]
        return np.clip(127 + 100 * np.sin(yy / 5.0) * np.cos(xx / 7.0) + rs.normal(0, 8, shape), 0, 255).astype(np.float32)
    if kind == "binary":
        return (rs.randint(0, 2, shape) * 255).astype(np.float32)
    assert kind == "nested"                                    # rectangles 255 / 0 / 128 inside one another
    img = np.full(shape, 255, np.float32)
    img[rows // 6:rows - rows // 6, cols // 6:cols - cols // 6] = 0
    img[rows // 3:rows - rows // 3, cols // 3:cols - cols // 3] = 128
    return img


def sweep_groups():
    """(kind, shape) -> list of cases: every sweep parameter set, and PROMOTE on 130 x 130"""
    out = {}
    for ki, kind in enumerate(SWEEP_KINDS):
        for si, shape in enumerate(SWEEP_SHAPES):
            img = sweep_image(kind, shape, 1000 + 20 * ki + si)
            assert img.size >= MIN_PIXELS
            sets = SWEEP_PARAMS + ([PROMOTE] if shape == (130, 130) else [])
            out["%s_%dx%d" % ((kind,) + shape)] = [("%s_%dx%d/p%d" % (kind, shape[0], shape[1], pi), img, kw) for pi, kw in enumerate(sets)]
    return out


def base_groups():
    """the images of tests/test_mser_cpu.py that the reference can be handed (1 x 37 and 23 x 1 are under 64 pixels) x PARAM_SETS"""
    out = {}
    for ii, img in enumerate(_images()):
        if img.size >= MIN_PIXELS:
            out["base_image%d" % ii] = [("base_image%d/p%d" % (ii, pi), img, kw) for pi, kw in enumerate(PARAM_SETS)]
    return out


# ---- planted structure -------------------------------------------------------------------------------------------------------

def _canvas(rows, cols, ground):
    return np.full((rows, cols), ground, np.float32)


def _merge_pair(size_a, size_b, level_a, level_b, vertical, wall=100, ground=200):
    """two basins side by side (or one above the other), a one-pixel wall of level `wall` between them: they meet AT the wall's
    level, where MergeRegions (getExtrema.cpp:267-361) keeps the one that was largest one level below and, on a tie, the first in
    the order up, left, right, down."""
    (ha, wa), (hb, wb) = size_a, size_b
    img = _canvas(max(ha, hb) + 6, wa + wb + 7, ground)
    img[3:3 + ha, 3:3 + wa] = level_a
    img[3:3 + min(ha, hb), 3 + wa] = wall
    img[3:3 + hb, 4 + wa:4 + wa + wb] = level_b
    return np.ascontiguousarray(img.T) if vertical else img


def _pinwheel(arms, equal_levels):
    """four one-pixel-wide arms that meet in ONE pixel from above, left, right and below: a four-way merge in one MergeRegions"""
    up, left, right, down = arms
    img = _canvas(up + down + 7, left + right + 7, 200)
    r, c = 3 + up, 3 + left
    lv = (20, 20, 20, 20) if equal_levels else (10, 20, 30, 40)
    img[r - up:r, c] = lv[0]
    img[r, c - left:c] = lv[1]
    img[r, c + 1:c + 1 + right] = lv[2]
    img[r + 1:r + 1 + down, c] = lv[3]
    img[r, c] = 100
    return img


def _blob(img, r0, c0, area, width, level):
    """`area` pixels of `level` in raster order inside a box `width` wide at (r0, c0)"""
    for k in range(area):
        img[r0 + k // width, c0 + k % width] = level


def _area_image(areas, ground=200, level=50, rows=40, cols=50):
    img = _canvas(rows, cols, ground)
    for i, a in enumerate(areas):
        _blob(img, 3 + 14 * (i // 3), 3 + 15 * (i % 3), a, 11, level)
    return img


def _edges_image():
    """regions that touch every edge and every corner of a 40 x 50 image (sizes differ, so a swap would show)"""
    img = _canvas(40, 50, 200)
    img[0:3, 0:4] = 30; img[0:4, 45:50] = 40; img[36:40, 0:5] = 50; img[35:40, 44:50] = 60      # the corners
    img[0:3, 20:27] = 70; img[37:40, 18:26] = 80; img[15:22, 0:3] = 90; img[14:23, 47:50] = 95  # the middle of every edge
    return img


def _rings(small_growth):
    """one seed, several stable levels: discs of radius 4, 8, 12, 16 at levels 20, 60, 100, 140 on a ground of 220; with small_growth a
    few pixels join between the levels, less than a tenth of the area (the near-equal-area rule of optThresh.cpp:41-62)"""
    yy, xx = np.mgrid[:48, :52]
    d2 = (yy - 24) ** 2 + (xx - 26) ** 2
    img = _canvas(48, 52, 220)
    for rad, lv in ((16, 140), (12, 100), (8, 60), (4, 20)):
        img[d2 < rad * rad] = lv
    if small_growth:
        img[24, 30] = 35; img[24, 31] = 45; img[23, 34] = 75; img[24, 35] = 85; img[24, 38] = 120
    return img


def _high_levels():
    """the highest stable threshold there is: a block at 253 on 255 with min_margin 1 gives pos 253, margin 2, thresh 254 (255 itself
    cannot occur, see the module's docstring); beside it a block at 250 (thresh 252) and one at 1 on the same ground"""
    img = _canvas(30, 40, 255)
    img[3:9, 3:10] = 253; img[3:9, 15:22] = 250; img[15:22, 5:12] = 1; img[15:21, 20:30] = 254
    return img


def _promote_image():
    """130 x 130: a striped dark region (three dark rows, one bright, a dark spine in column 0) whose first 9990 pixels are at level 10,
    the next 20 at 12 and the rest at 20, on 200.  It reaches 10000 pixels -- promoteAt = min(10000, min_size) -- at level 12 and
    min_size = 12000 only at level 20; its perimeter is larger than the growth at level 20, so the margin at level 12 runs on to 200 and
    the key's response tells from which level the region's record was kept."""
    img = _canvas(130, 130, 200)
    dark = (np.arange(130) % 4 != 3)[:, None] & np.ones((1, 130), bool)
    dark[:, 0] = True
    idx = np.flatnonzero(dark.ravel())
    assert len(idx) > 12000
    flat = img.reshape(-1)
    flat[idx[:9990]] = 10; flat[idx[9990:10010]] = 12; flat[idx[10010:]] = 20
    return img


def tie_image():
    """72 dark blocks of 6 x 6 on a ground of 150: 48 at level 50 and 24 at level 100 -- margins 100 (48 times) and 50 (24 times)"""
    img = _canvas(6 * 9 + 3, 12 * 9 + 3, 150)
    for k in range(72):
        r, c = 3 + 9 * (k // 12), 3 + 9 * (k % 12)
        img[r:r + 6, c:c + 6] = 50 if k < 48 else 100
    return img


def float_params_image():
    """ten dark blocks of 6 x 6 on 150: seven at level 50 (margin 100) and three at level 80 (margin 70)"""
    img = _canvas(12, 10 * 9 + 3, 150)
    for k in range(10):
        img[3:9, 3 + 9 * k:9 + 9 * k] = 50 if k < 7 else 80
    return img


# ExtremaParams::rel_threshold and rel_reg_number are FLOATS (extremaParams.h:68-70): 0.7f is 0.699999988, so RELATIVE_REG_NUMBER keeps
# floor(0.7f x 10) = 6 of ten keys where a double 0.7 would keep 7, and RELATIVE_TH's probe 100 x 0.7f = 69.9999988 keeps the keys of
# margin 70 (`>`), which a probe of 70.0 would drop.  0.1f and 0.3f lie ABOVE 0.1 and 0.3 and change nothing.
FLOAT_PARAMS = [dict(mode=3, rel_reg_number=0.7), dict(mode=1, rel_threshold=0.7), dict(mode=3, rel_reg_number=0.3),
                dict(mode=3, rel_reg_number=0.1), dict(mode=1, rel_threshold=0.3)]


# Every export mode on the tie image.  The cut falls INSIDE a run of equal margins, and which of the equal keys stay is decided by
# std::sort alone: this is comparable only because both sides run the same libstdc++ std::sort with the same comparison on the same
# sequence (MSER+ keys in region order, then MSER-).  Modes 1 and 4 cut with lower_bound at a response, which cannot split equal
# responses; there the threshold sits exactly ON the lower tie (0.5 x 100 = 50: `>` keeps none of the 50s), and mode 4's fixed
# threshold of 1.0 lies below every response, so its cut is reg_number or nothing.
TIE_PARAMS = [dict(mode=2, reg_number=17), dict(mode=2, reg_number=60), dict(mode=2, reg_number=60, tilt=3.0),
              dict(mode=2, reg_number=200, zoom=0.25), dict(mode=3, rel_reg_number=0.3), dict(mode=3, rel_reg_number=0.75),
              dict(mode=1, rel_threshold=0.5), dict(mode=1, rel_threshold=0.49), dict(mode=4, reg_number=31),
              dict(mode=4, reg_number=500), dict(mode=0, min_margin=50.0), dict(mode=0, min_margin=49.0),
              # no cut at all (reg_number < 0), mode 4 with fewer asked than found, and a relative number above 1: std::vector::resize
              # then APPENDS value-initialised keys (all fields zero) on both sides
              dict(mode=2, reg_number=-5), dict(mode=4, reg_number=5), dict(mode=3, rel_reg_number=1.5)]
TIE_BASE = dict(min_size=10, max_area=0.01)


def planted_groups():
    small = dict(min_size=5, max_area=1.0, min_margin=8.0)
    out = {}

    def add(group, name, img, kws, invert=True):
        lst = out.setdefault(group, [])
        for pi, kw in enumerate(kws):
            lst.append(("%s/%s/p%d" % (group, name, pi), img, kw))
            if invert:                                         # the same image inverted: the MSER- branch walks it as MSER+ did
                lst.append(("%s/%s_inverted/p%d" % (group, name, pi), (255 - img).astype(np.float32), kw))

    # the survivor rule at a merge on one grey level: equal and unequal areas, both raster orders, both directions, basins of one or
    # of two levels; min_size 5 makes regions of all of them, min_size 50 leaves them packed counters when they meet
    for vertical in (False, True):
        for sa, sb in (((6, 6), (6, 6)), ((6, 6), (6, 7)), ((6, 7), (6, 6)), ((5, 8), (8, 5)), ((4, 4), (9, 9)), ((9, 9), (4, 4))):
            for la, lb in ((10, 10), (10, 20), (20, 10)):
                add("merge", "pair_%dx%d_%dx%d_l%d_l%d_%s" % (sa + sb + (la, lb, "v" if vertical else "h")),
                    _merge_pair(sa, sb, la, lb, vertical), [small, dict(small, min_size=50)], invert=False)
    for arms in ((5, 5, 5, 5), (5, 6, 7, 8), (8, 7, 6, 5), (6, 9, 5, 9)):
        for eq in (True, False):
            add("merge", "pinwheel_%d_%d_%d_%d_%s" % (arms + ("eq" if eq else "ne",)), _pinwheel(arms, eq),
                [dict(small, min_size=3), dict(small, min_size=6)])
    # regions on the image border
    add("border", "edges_corners", _edges_image(), [dict(min_size=5, max_area=0.2, min_margin=8.0), LOOSE, dict(relative=1, min_margin=3.0, min_size=5)])
    # max_area: 40 x 50 x 0.05 = 100 pixels exactly; `cummulAreas[thresh] <= max_size` (optThresh.cpp:132) keeps 100 and drops 101
    assert int(40 * 50 * 0.05) == 100
    add("area", "max_area_99_100_101", _area_image((99, 100, 101)), [dict(min_size=30, max_area=0.05, min_margin=8.0)])
    # min_size: `cummulAreas[thresh] > min_size` keeps 31 of 29, 30, 31; 29 + 1 + 1 pixels at three levels pass through the promotion
    add("area", "min_size_29_30_31", _area_image((29, 30, 31)), [dict(min_size=30, max_area=0.5, min_margin=8.0)])
    grow = _area_image((29, 30, 31))
    grow[3 + 2, 3 + 7] = 60; grow[3 + 2, 3 + 8] = 70; grow[3 + 2, 18 + 8] = 60
    add("area", "min_size_growing", grow, [dict(min_size=30, max_area=0.5, min_margin=8.0), dict(min_size=30, max_area=0.5, min_margin=5.0)])
    # thresholds at the top of the byte
    add("levels", "high_levels", _high_levels(), [dict(min_size=5, max_area=1.0, min_margin=1.0), dict(min_size=5, max_area=1.0, min_margin=2.0)])
    # one seed, several stable levels
    for sg in (False, True):
        add("levels", "rings_%d" % sg, _rings(sg), [dict(min_size=5, max_area=1.0, min_margin=8.0), dict(min_size=5, max_area=1.0, min_margin=3.0),
                                                     dict(min_size=5, max_area=1.0, min_margin=3.0, relative=1)])
    # promotion below min_size
    add("promote", "striped_130x130", _promote_image(), [PROMOTE, dict(PROMOTE, min_size=10000), dict(PROMOTE, min_size=9000)])
    # ties at the export cut
    add("ties", "blocks72", tie_image(), [dict(TIE_BASE, **kw) for kw in TIE_PARAMS], invert=False)
    add("ties", "float_params", float_params_image(), [dict(TIE_BASE, max_area=0.05, **kw) for kw in FLOAT_PARAMS])
    return out


def trunc_block_cases():
    """every planted value of mser_front_cases.TRUNC_VALUES, 17.9 and 200.5 as a 10 x 11 block on a constant 40 x 53 ground, two
    grounds, two places: the reference's own (unsigned char)float decides what the block is"""
    out = []
    values = np.concatenate([TRUNC_VALUES, np.float32([17.9, 200.5])])
    for vi, v in enumerate(values):
        for ground in (60.0, 200.0):
            for r0, c0 in ((5, 7), (29, 41)):
                img = _canvas(40, 53, ground)
                img[r0:r0 + 10, c0:c0 + 11] = v
                out.append(("trunc/v%d_g%d_r%d" % (vi, ground, r0), img, dict(min_size=10, max_area=0.5, min_margin=5.0)))
    return out


def all_groups():
    """group name -> cases, for the product and the restatement alike"""
    out = {}
    out.update(base_groups())
    out.update(sweep_groups())
    out.update(planted_groups())
    tr = trunc_block_cases()
    for k in range(0, len(tr), 26):
        out["trunc_blocks_%d" % (k // 26)] = tr[k:k + 26]
    return out


def split_kw(kw):
    """-> (the detector's keywords, tilt, zoom)"""
    kw = dict(kw)
    tilt, zoom = kw.pop("tilt", 1.0), kw.pop("zoom", 1.0)
    return kw, tilt, zoom


def gpu_suite_cases(oracle):
    """the images on which the GPU suite compares the device paths with oracle.detect_msers / detect_describe_views(mser=...): the
    session's small pair, the single-view cases of tests/test_gpu_mser_front.py and test_gpu_parity.py, and -- synthesised by the
    oracle, as detect_describe_views does it -- every view of the engine cases and of test_mser_device_path_and_view_loop"""
    import mser_front_cases as MC
    from mods_amd import synthetic
    a, b, _ = synthetic.make_pair(rows=240, cols=320, nblobs=420, seed=777)            # conftest.small_pair
    default = dict(min_size=30, max_area=0.05, min_margin=8.0)
    out = [("small_pair/a", a, {}), ("small_pair/b", b, {}),
           ("degenerate/blank", np.full((96, 128), 90, np.float32), {}),
           ("degenerate/tiny_9x11", np.random.RandomState(1).uniform(0, 255, (9, 11)).astype(np.float32), {})]
    for name, img in MC.trunc_cases().items():
        out.append(("front_trunc/" + name, img, MC.MSER_LOOSE))

    def views_of(tag, image, views, kw):
        for vi, v in enumerate(views):
            img, _, ident = oracle.synth_view(image, v)
            tz = {} if ident else dict(tilt=abs(v.tilt), zoom=v.zoom)
            if img.size >= MIN_PIXELS:
                out.append(("%s/view%d" % (tag, vi), img, dict(kw, **tz)))

    views_of("view_loop", a, oracle.set_vs_pars([1.0], [1, 2], 360.0, 0.8, 1, []), default)
    for name, case in MC.engine_cases().items():
        views_of("engine/" + name, case["image"], oracle.set_vs_pars(case["scales"], case["tilts"], case["phi"], case["sigma"], 1, []),
                 case["mser"])
    return out
