"""Inputs of the reference-pin tests (tests/test_ref_pin_cpu.py, tests/test_gpu_ref_pin.py) that no other case module has: operands
of atan2LUTff, calls of interpolate / interpolateCheckBorders, inputs of the 2x2 / 3x3 helpers, further Baumberg jobs and regions
for the planes on which too few of baumberg_cases' / affshape_cases' converge (and DetectAffineShape put together from the
reference's parts), and the sampling calls of the describe_cases regions.  All fixed-seed numpy; no GPU in here, and the oracle
module only where a caller hands it in.  Every list carries the SITUATIONS it was built for as tags; tests/test_ref_pin_cpu.py
asserts from the reference's own answers that each of them occurs.
"""
import functools
import math

import numpy as np

F = np.float32
FMAX = np.finfo(F).max


def _ulps(v, k):
    """v moved k f32 steps (k may be negative)"""
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
    return v


# ---- atan2LUTff --------------------------------------------------------------------------------------------------------------------
OCTANTS = ((1, 1, 0), (1, 1, 1), (1, -1, 0), (1, -1, 1), (-1, 1, 0), (-1, 1, 1), (-1, -1, 0), (-1, -1, 1))     # sign x, sign y, swapped


def lut_index(small, big):
    """(int)(255.f * small / big) in f32, as atan2LUTff forms its table index from two positive f32 numbers"""
    with np.errstate(all="ignore"):
        return int(F(F(255.0) * F(small)) / F(big))


@functools.lru_cache(maxsize=None)
def atan2_cases():
    """-> (yx f32 [n, 2], tags: list of sets).  Tags: zero_pp / zero_pn / zero_np / zero_nn (signs of y, x), axis, diagonal,
    cell(i, o, side) for table cell boundary i in 1..255 of octant o with the index below (side 0) / at (side 1) the boundary,
    subnormal, one_inf, refused_nan, refused_two_inf, refused_overflow."""
    yx, tags = [], []

    def add(y, x, *t):
        yx.append((F(y), F(x)))
        tags.append(set(t))

    for sy, ny in ((0.0, "p"), (-0.0, "n")):
        for sx, nx in ((0.0, "p"), (-0.0, "n")):
            add(sy, sx, "zero_" + ny + nx)
    for v in (1.0, 1e-30, 1e36, 2.5):
        for z in (0.0, -0.0):
            for s in (1.0, -1.0):
                add(z, s * v, "axis")
                add(s * v, z, "axis")
    for v in (1.0, 255.0, 1e-20, 7.3, 1e-45, 2.0 ** 100):
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                add(sy * v, sx * v, "diagonal")
    # every cell boundary: big = b, small = the f32 nearest i * b / 255 and its neighbours two steps either way.  Index 255 is
    # reached with small == big where the octant's comparison is not strict (the swapped octants) and, where it is strict, only by
    # a quotient that rounds up to 255.0: orient_cases.BIG_IDX255 = (0.99231726, its predecessor)
    for b in (255.0, 1.0, 3.7, 0.99231726):
        for i in range(1, 256):
            s0 = F(np.float64(i) * np.float64(F(b)) / 255.0)
            for k in (-2, -1, 0, 1, 2):
                small = _ulps(s0, k)
                if not (0 < small <= F(b)):
                    continue
                idx = lut_index(small, F(b))
                side = None if idx not in (i - 1, i) else idx - (i - 1)
                for o, (sx, sy, swap) in enumerate(OCTANTS):
                    if small == F(b) and not swap:
                        continue                      # |x| == |y| belongs to the swapped octants
                    x, y = (small, F(b)) if swap else (F(b), small)
                    add(sy * y, sx * x, *(() if side is None else (("cell", i, o, side),)))
    sub = np.array([1, 2, 0x7FFFFF, 0x400000], np.uint32).view(F)
    for a in sub:
        for c in (sub[1], F(1e-38), F(1.0), sub[2]):
            for sy in (1.0, -1.0):
                for sx in (1.0, -1.0):
                    add(sy * a, sx * c, "subnormal")
                    add(sy * c, sx * a, "subnormal")
    for v in (0.0, 1.0, -3.0, 1e30):
        for inf in (np.inf, -np.inf):
            add(v, inf, "one_inf")
            add(inf, v, "one_inf")
    for v in (0.0, 1.0, -1.0, np.inf, np.nan):
        add(np.nan, v, "refused_nan")
        add(v, np.nan, "refused_nan")
    for sy in (np.inf, -np.inf):
        for sx in (np.inf, -np.inf):
            add(sy, sx, "refused_two_inf")
    for v in (FMAX, -FMAX, FMAX / F(128.0)):
        add(v, 1.0, "refused_overflow")
        add(1.0, v, "refused_overflow")
    return np.array(yx, F).reshape(-1, 2), tags


ATAN2_REFUSED = ("refused_nan", "refused_two_inf", "refused_overflow")


# ---- interpolate and its border checks -----------------------------------------------------------------------------------------------
INTERP_SHAPES = ((3, 3), (19, 23), (57, 83))            # rows, cols
INTERP_RES = ((19, 19), (41, 41), (3, 3), (5, 9), (9, 5))


@functools.lru_cache(maxsize=None)
def interp_images():
    rs = np.random.RandomState(6101)
    out = []
    for r, c in INTERP_SHAPES:
        y, x = np.mgrid[0:r, 0:c].astype(np.float64)
        img = (120.0 + 60.0 * np.sin(0.4 * x + 0.2) * np.cos(0.3 * y) + rs.uniform(-30.0, 30.0, (r, c))).astype(F)
        img.setflags(write=False)
        out.append(img)
    return out


@functools.lru_cache(maxsize=None)
def interp_calls():
    """-> list of dict(img (index), par (ofsx, ofsy, a11, a12, a21, a22 as f32), res (rows, cols), centre, window): centre in
    inside / edge_left / edge_right / edge_top / edge_bottom / outside, window in small / medium / large (the matrix' size, which
    with the centre decides whether the window lies inside, straddles the border or lies outside)"""
    rs = np.random.RandomState(6102)
    calls = []
    for ii, (rows, cols) in enumerate(INTERP_SHAPES):
        centres = {"inside": [(0.5 * cols - 0.3, 0.5 * rows + 0.2), (0.5 * cols, 0.5 * rows), (0.37 * cols, 0.61 * rows)],
                   "edge_left": [(0.0, 0.5 * rows), (1.0, 0.4 * rows)], "edge_right": [(cols - 1.0, 0.5 * rows), (cols - 2.0, 0.6 * rows)],
                   "edge_top": [(0.5 * cols, 0.0), (0.45 * cols, 1.0)], "edge_bottom": [(0.5 * cols, rows - 1.0), (0.55 * cols, rows - 2.0)],
                   "outside": [(-30.0, 0.5 * rows), (cols + 30.0, 0.5 * rows), (0.5 * cols, -30.0), (0.5 * cols, rows + 30.0),
                               (-1.5, -1.5), (cols + 0.5, rows + 0.5)]}
        for cname, lst in centres.items():
            for (cx, cy) in lst:
                for res in INTERP_RES:
                    half = max(res) // 2 + 1
                    reach = {"small": 0.02 * min(rows, cols) / half, "medium": 0.3 * min(rows, cols) / half, "large": 1.5 * max(rows, cols) / half}
                    for wname, k in reach.items():
                        for _ in range(2):
                            t = rs.uniform(-math.pi, math.pi)
                            k1, k2 = k * rs.uniform(0.7, 1.4), k * rs.uniform(0.7, 1.4)
                            A = (k1 * math.cos(t), -k2 * math.sin(t), k1 * math.sin(t), k2 * math.cos(t))
                            jit = rs.uniform(-0.4, 0.4, 2) if cname in ("inside", "outside") else (0.0, 0.0)
                            calls.append(dict(img=ii, par=tuple(F(v) for v in (cx + jit[0], cy + jit[1]) + A), res=res, centre=cname,
                                              window=wname))
    # axis-aligned unit steps on integer centres: every sample on a pixel, zero weights
    for ii, (rows, cols) in enumerate(INTERP_SHAPES):
        for res in ((3, 3), (5, 9)):
            calls.append(dict(img=ii, par=tuple(F(v) for v in (cols // 2, rows // 2, 1.0, 0.0, 0.0, 1.0)), res=res, centre="inside",
                              window="unit"))
    return calls


def check_rows(calls):
    """the [n, 10] rows pyoracle.ref_interpolate_check_borders takes, for interp calls"""
    return np.array([[INTERP_SHAPES[c["img"]][1], INTERP_SHAPES[c["img"]][0]] + [float(v) for v in c["par"]] + [c["res"][1], c["res"][0]]
                     for c in calls], np.float64)


@functools.lru_cache(maxsize=None)
def check_only_rows():
    """further interpolateCheckBorders calls [n, 10], with the result sizes DetectOrientation, ReprojectRegions and
    DetectAffineShape pass -- even ones, 0 and negative ones included (only interpolate itself needs odd sizes) -- and corners
    planted on the compared values: floor(imx) <= 0 at 1 and one step below 1, ceil(imx) >= width at cols - 3 and one step above"""
    rs = np.random.RandomState(6103)
    rows = []
    for (h, w) in INTERP_SHAPES + ((240, 320), (768, 1024)):
        for _ in range(150):
            s = rs.uniform(0.2, 0.3 * min(h, w))
            t = rs.uniform(-math.pi, math.pi)
            A = (math.cos(t) * rs.uniform(0.3, 2), -math.sin(t) * rs.uniform(0.3, 2), math.sin(t) * rs.uniform(0.3, 2), math.cos(t) * rs.uniform(0.3, 2))
            res = int(rs.choice([0, 1, 2, 3, 4, 7, 10, 19, 20, 41, -3, int(s)]))
            rows.append([w, h, rs.uniform(-3, w + 3), rs.uniform(-3, h + 3)] + list(A) + [res, int(rs.choice([res, res + 1, 3]))])
        for res in (2, 4, 19):                       # identity matrix: corner = centre -+ ceil(res / 2)
            hw = math.ceil(res / 2.0)
            for base, axis in ((1.0 + hw, 0), (w - 3.0 - hw, 0), (1.0 + hw, 1), (h - 3.0 - hw, 1)):
                for k in (-1, 0, 1):
                    v = float(_ulps(base, k))
                    cx, cy = (v, 0.5 * h) if axis == 0 else (0.5 * w, v)
                    rows.append([w, h, cx, cy, 1.0, 0.0, 0.0, 1.0, res, res])
    a = np.array(rows, np.float64)
    a[:, 2:8] = a[:, 2:8].astype(F).astype(np.float64)
    return a


# ---- the 2x2 / 3x3 helpers -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inv_sqrt_cases():
    """-> list of (tag, (a, b, c)): the symmetric 2x2 matrix [[a, b], [b, c]] handed to invSqrt"""
    rs = np.random.RandomState(6201)
    out = [("isotropic", (v, 0.0, v)) for v in (1.0, 0.25, 37.5, 1e-12, 1e12)]
    out += [("diagonal", (a, 0.0, c)) for a, c in ((1.0, 4.0), (9.0, 0.5), (1e-6, 1e3))]
    out += [("equal_diagonal", (2.0, b, 2.0)) for b in (0.5, -0.5, 1e-20)]                     # r = 0
    out += [("tiny_b", (3.0, b, 1.0)) for b in (1e-30, -1e-38, float(np.array([1], np.uint32).view(F)[0]))]
    for _ in range(12):                                                                         # a c - b^2 within a few ulps of 0
        a, c = rs.uniform(0.5, 50.0, 2)
        b = math.sqrt(a * c) * rs.choice([-1.0, 1.0])
        out.append(("nearly_singular", (a, float(_ulps(b, int(rs.randint(-3, 4)))), c)))
    out += [("singular", (1.0, 1.0, 1.0)), ("singular", (4.0, -2.0, 1.0)), ("zero", (0.0, 0.0, 0.0)), ("zero", (0.0, 0.0, 5.0))]
    out += [("indefinite", (1.0, 3.0, 1.0)), ("indefinite", (-2.0, 0.5, 1.0)), ("negative_definite", (-2.0, 0.3, -1.0))]
    out += [("nan", (np.nan, 0.5, 1.0)), ("nan", (1.0, np.nan, 1.0)), ("nan", (1.0, 0.5, np.nan)), ("inf", (np.inf, 0.5, 1.0)),
            ("inf", (1.0, np.inf, 1.0))]
    for _ in range(200):
        e = rs.uniform(-6, 6)
        l1, l2 = 10.0 ** e * rs.uniform(0.2, 5.0), 10.0 ** e * rs.uniform(0.2, 5.0)
        t = rs.uniform(-math.pi, math.pi)
        cs, sn = math.cos(t), math.sin(t)
        out.append(("random", (cs * cs * l1 + sn * sn * l2, cs * sn * (l1 - l2), sn * sn * l1 + cs * cs * l2)))
    return [(t, tuple(float(F(v)) for v in abc)) for t, abc in out]


@functools.lru_cache(maxsize=None)
def eigen_cases():
    """-> list of (tag, (a, b, c, d)) for getEigenvalues of [[a, b], [c, d]]"""
    rs = np.random.RandomState(6202)
    out = [("isotropic", (v, 0.0, 0.0, v)) for v in (1.0, 0.3, 1e20, 1e-30)]
    out += [("negative_discriminant", m) for m in ((0.0, -1.0, 1.0, 0.0), (1.0, -2.0, 2.0, 1.0), (0.5, 3.0, -3.0, 0.7))]
    for _ in range(10):                        # discriminant within a few ulps of 0 on either side: a = d, b c = -+tiny
        a = rs.uniform(0.5, 3.0)
        e = float(F(10.0) ** F(rs.randint(-44, -8)))
        out.append(("nearly_zero_discriminant", (a, e, rs.choice([-1.0, 1.0]) * e, a)))
        out.append(("nearly_zero_discriminant", (a, 1.0, float(_ulps(0.0, int(rs.randint(-2, 3)))), float(_ulps(a, int(rs.randint(-2, 3)))))))
    out += [("nearly_singular", (1.0, 2.0, 0.5, float(_ulps(1.0, k)))) for k in (-2, -1, 0, 1, 2)]
    out += [("nan", (np.nan, 0.0, 0.0, 1.0)), ("nan", (1.0, np.nan, 0.0, 1.0)), ("nan", (1.0, 0.0, 0.0, np.nan)), ("inf", (np.inf, 0.0, 0.0, 1.0)),
            ("overflow", (3e38, 0.0, 0.0, 3e38))]
    out += [("random", tuple(rs.uniform(-3, 3, 4))) for _ in range(200)]
    return [(t, tuple(float(F(v)) for v in m)) for t, m in out]


@functools.lru_cache(maxsize=None)
def solve3_cases():
    """-> list of (tag, A [9], b [3]) for solveLinear3x3; pivot_row0/1/2: where the largest |A[i][0]| is; swap2: the second pivot
    search swaps rows 1 and 2"""
    rs = np.random.RandomState(6203)
    out = []
    for _ in range(150):
        out.append(("random", rs.uniform(-5, 5, 9), rs.uniform(-5, 5, 3)))
    for row in range(3):
        for _ in range(6):
            A = rs.uniform(-1, 1, 9)
            A[3 * row] = rs.choice([-1.0, 1.0]) * rs.uniform(4, 9)
            out.append(("pivot_row%d" % row, A, rs.uniform(-5, 5, 3)))
    out.append(("tie_pivot", np.array([2.0, 1, 0, -2.0, 3, 1, 2.0, 0, 5]), np.array([1.0, 2, 3])))
    out.append(("isotropic", np.array([2.0, 0, 0, 0, 2.0, 0, 0, 0, 2.0]), np.array([1.0, -2, 3])))
    out.append(("singular", np.array([1.0, 2, 3, 2, 4, 6, 1, 0, 1]), np.array([1.0, 2, 3])))
    out.append(("singular", np.zeros(9), np.array([1.0, 2, 3])))
    out.append(("nearly_singular", np.array([1.0, 2, 3, 4, 5, 6, 7, 8, float(_ulps(9.0, 1))]), np.array([1.0, 0, -1])))
    out.append(("nan", np.array([np.nan, 2, 3, 4, 5, 6, 7, 8, 10.0]), np.array([1.0, 0, -1])))
    out.append(("nan", np.array([1.0, 2, 3, 4, 5, 6, 7, 8, 10.0]), np.array([1.0, np.nan, -1])))
    return [(t, np.asarray(A, F), np.asarray(b, F)) for t, A, b in out]


@functools.lru_cache(maxsize=None)
def rectify_cases():
    """-> list of (tag, (a11, a12, a21, a22)) doubles for rectifyAffineTransformationUpIsUp"""
    rs = np.random.RandomState(6204)
    out = [("isotropic", (v, 0.0, 0.0, v)) for v in (1.0, 0.1, 250.0)]
    out += [("rotation", (math.cos(t), -math.sin(t), math.sin(t), math.cos(t))) for t in (0.3, 1.5707963, 3.0, -2.0)]
    out += [("reflection", (1.0, 0.0, 0.0, -1.0)), ("reflection", (0.5, 2.0, 2.0, 0.5))]
    out += [("nearly_singular", (1.0, 2.0, 0.5, float(np.nextafter(1.0, 2.0)))), ("nearly_singular", (1.0, 2.0, 0.5, float(np.nextafter(1.0, 0.0))))]
    out += [("singular", (1.0, 2.0, 0.5, 1.0)), ("zero_first_row", (0.0, 0.0, 1.0, 1.0)), ("zero", (0.0, 0.0, 0.0, 0.0))]
    out += [("nan", (np.nan, 0.0, 0.0, 1.0)), ("nan", (1.0, 0.0, np.nan, 1.0)), ("inf", (np.inf, 0.0, 0.0, 1.0))]
    out += [("random", tuple(rs.uniform(-3, 3, 4) * 10.0 ** rs.uniform(-3, 3))) for _ in range(300)]
    return [(t, tuple(float(v) for v in m)) for t, m in out]


@functools.lru_cache(maxsize=None)
def gradient_images():
    """images for computeGradient / computeGradientMagnitudeAndOrientation: 2 x 2 (only one-sided differences), 3 x 3, 19 x 19,
    41 x 41, 7 x 30; values with full mantissas, a flat one, one with exact ties (|xg| == |yg|)"""
    rs = np.random.RandomState(6205)
    out = [("tiny", rs.uniform(0, 255, (2, 2))), ("three", rs.uniform(0, 255, (3, 3))), ("window", rs.uniform(0, 255, (19, 19))),
           ("patch", rs.standard_normal((41, 41)) * 60), ("wide", rs.uniform(-1e-3, 1e-3, (7, 30))), ("flat", np.full((9, 9), 90.0)),
           ("ties", np.add.outer(np.arange(11.0), np.arange(11.0)) * 3.0), ("large", rs.uniform(-1e30, 1e30, (8, 8)))]
    return [(t, np.ascontiguousarray(a, F)) for t, a in out]


# ---- extra Baumberg jobs and regions ----------------------------------------------------------------------------------------------------
# tests/test_ref_pin_cpu.py requires the reference to converge on a quarter of the jobs of every plane.  On three of baumberg_cases'
# planes (the 33 x 47 blob plane, the constant plane and the ridge plane) and on two of affshape_cases' images it converges on fewer.
# What converges there at a high rate are LARGE windows around the middle: at 6 to 8 times the base scale the 19 x 19 window spans
# the whole plane, zeros outside included, and sees the plane as one blob.  For DetectAffineShape the region's own matrix is made
# small, so that the up-front border test passes while the loop's windows (which start from the identity) leave the image.
EXTRA_BAUMBERG = {1: 100, 3: 100, 4: 100}           # plane of baumberg_cases -> further jobs
EXTRA_AFFSHAPE = {1: (60, (3.0, 4.0, 6.0)), 2: (70, (2.0,))}      # image of affshape_cases -> (further regions, scale factors)


def extra_baumberg_jobs(shapes):
    """shapes = baumberg_cases.plane_shapes() -> (plane_of, xyspd) of the further jobs, planes interleaved"""
    rs = np.random.RandomState(6301)
    po, xy = [], []
    for k in range(max(EXTRA_BAUMBERG.values())):
        for p, count in sorted(EXTRA_BAUMBERG.items()):
            if k < count:
                rows, cols = shapes[p]
                pd, f = float(rs.choice([1.0, 2.0])), float(rs.choice([6.0, 8.0]))
                lx, ly = rs.uniform(0.25 * cols, 0.75 * cols), rs.uniform(0.25 * rows, 0.75 * rows)
                po.append(p)
                xy.append((lx * pd, ly * pd, 1.6 * f * pd, pd))
    return np.array(po, np.int32), np.array(xy, F).reshape(-1, 4)


def extra_affshape_regions(dtype, shapes):
    """shapes = affshape_cases.SHAPES, dtype = its REGION -> {image: REGION array} of the further regions (scales that are f32
    numbers, as affshape_model requires)"""
    rs = np.random.RandomState(6302)
    out = {}
    for i, (count, factors) in sorted(EXTRA_AFFSHAPE.items()):
        rows, cols = shapes[i]
        a = np.zeros(count, dtype)
        a["img_id"], a["type"], a["id"] = i, 6, np.arange(count)
        k = a["det_kp"]
        t, m = rs.uniform(0, math.pi, count), rs.uniform(0.01, 0.03, count)
        k["x"], k["y"] = rs.uniform(0.3 * cols, 0.7 * cols, count), rs.uniform(0.3 * rows, 0.7 * rows, count)
        k["s"] = [float(F(F(1.6) * F(factors[q]))) for q in rs.randint(0, len(factors), count)]
        k["a11"], k["a12"], k["a21"], k["a22"] = m * np.cos(t), -m * np.sin(t), m * np.sin(t), m * np.cos(t)
        k["response"] = rs.uniform(0.0, 1.0, count)
        a["reproj_kp"] = a["det_kp"]
        a.setflags(write=False)
        out[i] = a
    return out


# ---- the job lists of the Baumberg comparisons, and DetectAffineShape from the reference's parts ----------------------------------------
def _bc():
    from tests import baumberg_cases
    return baumberg_cases


def _ac():
    from tests import affshape_cases
    return affshape_cases


def _am():
    from tests import affshape_model
    return affshape_model


def baumberg_jobs():
    """baumberg_cases.jobs() followed by ref_pin_cases' further jobs"""
    po, xy = _bc().jobs()
    epo, exy = extra_baumberg_jobs(_bc().plane_shapes())
    return np.concatenate([po, epo]), np.concatenate([xy, exy])


def affshape_lists():
    """affshape_cases.regions() with ref_pin_cases' further regions appended to images 1 and 2"""
    extra = extra_affshape_regions(_ac().REGION, _ac().SHAPES)
    out = []
    for i, regs in enumerate(_ac().regions()):
        if i in extra:
            e = extra[i].copy()
            e["id"] += len(regs)
            regs = np.concatenate([regs, e])
        out.append(regs)
    return out


def reference_affshape(oracle, img, regs, **params):
    """DetectAffineShape from the reference's parts: its interpolateCheckBorders (int overload, with affshape_model's ratio and
    res: synth-detection.cpp:950-964 is not in the pinned files) decides who runs, its findAffineShape runs them at
    pixelDistance 1 and initialSigma 1.6.  -> dict(border, hit, u, iters) per input region"""
    _am().assert_f32_scales(regs)
    k = regs["det_kp"]
    _, res = _am().ratio_res(k["s"])
    f = lambda a: a.astype(F).astype(np.float64)          # noqa: E731
    n = len(regs)
    t = np.stack([np.full(n, img.shape[1], np.float64), np.full(n, img.shape[0], np.float64), f(k["x"]), f(k["y"]), f(k["a11"]), f(k["a12"]),
                  f(k["a21"]), f(k["a22"]), res.astype(np.float64), res.astype(np.float64)], 1)
    border = oracle.ref_interpolate_check_borders(t)
    idx = np.nonzero(~border)[0]
    out = dict(border=border, hit=np.zeros(n, np.int32), u=np.zeros((n, 4), F), iters=np.full(n, -1, np.int32))
    kk = k[idx]
    xyspd = np.stack([kk["x"].astype(F), kk["y"].astype(F), kk["s"].astype(F), np.ones(len(idx), F)], 1)
    r = oracle.ref_find_affine_shape_batch([img], np.zeros(len(idx), np.int32), xyspd, oracle.default_params(affInitialSigma=float(_am().SIGMA), **params))
    for name in ("hit", "u", "iters"):
        out[name][idx] = r[name]
    return out


# ---- the sampling calls of the describe_cases regions ---------------------------------------------------------------------------------
def sampling_call(kp, mr_size, fast, patch_size=41):
    """The interpolate() call DescribeRegions makes for keypoint record kp (x, y, a11 .. a22, s as doubles) when it samples the
    image straight into the patch: synth-detection.hpp:233-246 for fast, :186-190 and :213-222 for the direct branch of the slow
    path.  -> (ofsx, ofsy, a11, a12, a21, a22) as f32, or None when the slow path takes its smoothed branch (imageToPatchScale > 0.4)."""
    x, y, s = float(kp["x"]), float(kp["y"]), float(kp["s"])
    A = [F(float(kp[f])) for f in ("a11", "a12", "a21", "a22")]
    if fast:
        pis = 2 * int(mr_size * s) + 1
        sc = F(np.float64(pis) / np.float64(patch_size))
    else:
        mr_scale = F(math.ceil(s * mr_size))
        pis = 2 * int(mr_scale) + 1
        sc = F(pis) / F(patch_size)
        if float(sc) > 0.4:                      # the f32 scale against the double 0.4
            return None
    return (F(x), F(y)) + tuple(a * sc for a in A)


def window_call(kp):
    """the first interpolate() call of the smoothed branch (synth-detection.hpp:200-207): the region's own matrix, unscaled"""
    return tuple(F(float(kp[f])) for f in ("x", "y", "a11", "a12", "a21", "a22"))
