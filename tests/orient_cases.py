"""Inputs of the orientation parity tests (tests/test_orient_cases_cpu.py proves the claims, tests/test_gpu_orient.py runs them
through Context.detect_orientation).  No GPU in here.

The identity harness: at mr_size = 20.0 the measurement window is 2 * 20 + 1 = 41 px = the patch, so a region with s = 1, A = I
and an integer centre gets curr_sc = 1.0f, integer sample coordinates and zero bilinear weights: the 41 x 41 patch the kernel
sees is img[y - 20 : y + 21, x - 20 : x + 21] bit for bit.  `compose()` puts every planted patch into a cell of one f32 image and
lists one region per cell.

Planted patches (`planted()`; every record: name, family, patch [41, 41] f32, claim):
  ramps      I = (xg / 2) c + (yg / 2) r, exact in f32, one gradient everywhere: all 1245 votes in one bin.  big = 255, small =
             i + 0.5 puts 255 * small / big into table index i, for the 8 sign / octant codes x idx 0 .. 255; idx 255 is small =
             big where |x| > |y| is false, and where it is true (the quotient has to ROUND to 255) a planted gradient pair
             (x, pred(x)) found by search.  Named ramps: x == 0 with y < 0 (the special case, angle 0) and y > 0, angle exactly pi
             (x < 0, tiny y > 0: the unread bin 36) and exactly -pi (bin 0).
  extremes   flat (no votes); |gradient| exactly 1, one ulp above, and sqrt rounding down to 1; votes confined to ONE lane's 21
             consecutive entries of the voting list (three lanes); one row pair whose bins get 1, 7, 8 and 9 votes.
  peaks      built from FRAME SITES: the mask pixels next to the patch frame (row / column 1 and 39), whose outward neighbour
             is a frame pixel no other voting pixel reads.  A site takes any gradient whose inward component is at most 1 (its
             side effects then have magnitude <= 1 and do not vote), and its magnitude is searched so that mag * mask is EXACTLY
             a short dyadic T: single votes of exactly equal weight in chosen bins, all smoothing sums exact.  Centre bump,
             exact tie of two maxima, two-bin plateau, peaks at bins 0 and 35, plain / Half differing, a tie made by the fold,
             0 .. 5 peaks, unequal peaks in rising order, and 18 peaks (every even bin: the [1 1 1] smoothing keeps an
             alternating pattern's amplitude) -- the most a 36-bin histogram can have, so no search was needed: MAX_PEAKS = 18.
  random     smooth, white, low-contrast (|gradient| straddles 1) and integer-quantised noise.

Geometric cases (`geometric()`): explicit regions on a 200 x 260 blurred-noise image with negative values, each with the class it
claims per mr_size: "inside" (fast branch), "touch_inside" (bounds branch, every tap inside), "overhang" (passes the K_SIGMA box,
taps outside the image read 0), "dropped" (fails the box).  `small_image()`: a 30 x 30 image, smaller than the window.
"""
import numpy as np

import orient_model as M

F = np.float32
PS, HALF = 41, 20
MR_IDENTITY = 20.0
MR_SIZES = (1.0, 5.1962, 8.0, 20.0)
K_SIGMA = 2 * 3.0 * 3.0 ** 0.5
MAX_PEAKS = 18            # reached by peaks/alternating18 (the theoretical maximum: peaks are strict, so no two are adjacent)
RANDOM_PER_KIND = 75
BIG_IDX255 = (F(0.99231726), F(0.9923172))   # x, pred(x): 255 * pred(x) / x rounds to 255.0 although |x| > |y|

_planted = None


def ramp(xg, yg):
    """I = (xg / 2) c + (yg / 2) r: central differences xg, yg at every interior pixel (exact for the dyadic values used)"""
    r, c = np.mgrid[0:PS, 0:PS].astype(F)
    return (F(xg) / F(2)) * c + (F(yg) / F(2)) * r


def separable(xg_cols, yg_rows):
    """I = f(r) + g(c) with g(c + 1) - g(c - 1) = xg_cols[c], f(r + 1) - f(r - 1) = yg_rows[r]: the gradient of pixel (r, c) is
    (xg_cols[c], yg_rows[r])"""
    g, f = np.zeros(PS, F), np.zeros(PS, F)
    for k in range(1, PS - 1):
        g[k + 1] = g[k - 1] + F(xg_cols[k])
        f[k + 1] = f[k - 1] + F(yg_rows[k])
    return (f[:, None] + g[None, :]).astype(F)


# ---- frame sites ---------------------------------------------------------------------------------------------------------------
SITE_OFFSETS = (14, 17, 20, 23, 26)      # three apart: the pixels one site writes are read by no other site


def _sites():
    h = [("right", r) for r in SITE_OFFSETS] + [("left", r) for r in SITE_OFFSETS]
    v = [("top", c) for c in SITE_OFFSETS] + [("bottom", c) for c in SITE_OFFSETS]
    return h, v


def _site_pixel(edge, k):
    return {"right": (k, 39), "left": (k, 1), "top": (1, k), "bottom": (39, k)}[edge]


def _solve_mag(m, T, fixed, sign):
    """free component u of the given sign with fl(fl(sqrt(fl(u u) + fl(fixed fixed))) * m) == T exactly and the magnitude above 1"""
    s = float(T) / float(m)
    want = max(s * s - float(fixed) ** 2, 0.0) ** 0.5
    base = int(np.array([want], F).view(np.int32)[0])
    u = (base + np.arange(-60000, 60001, dtype=np.int64)).astype(np.int32).view(F)
    mag = np.sqrt(u * u + F(fixed) * F(fixed))
    hit = np.nonzero((mag * F(m) == F(T)) & (mag > F(1)))[0]
    assert len(hit), ("no gradient of weight", T, "at mask", m)
    pick = u[hit[np.argmin(np.abs(hit - 60000))]]
    return F(np.copysign(pick, sign))


def bin_angle(b):
    """an angle (degrees) well inside histogram bin b, kept 42 degrees or less off an axis so that a frame site can take it"""
    a = -175.0 + 10.0 * b
    if b % 9 == 4:                       # the bins around the diagonals: 3 degrees towards the horizontal
        a += 3.0 if (b // 9) % 2 else -3.0
    return a


def site_patch(votes):
    """votes: [(angle in degrees, T)] -> patch with one vote per entry, of weight exactly T, at a frame site"""
    hs, vs = _sites()
    p = np.zeros((PS, PS), F)
    mask = M.circular_gauss_mask()
    for ang, T in votes:
        ca, sa = np.cos(np.radians(ang)), np.sin(np.radians(ang))
        horizontal = abs(sa) <= abs(ca)
        edge, k = (hs if horizontal else vs).pop(0)
        r, c = _site_pixel(edge, k)
        s = float(T) / float(mask[r, c])
        if horizontal:
            y = F(np.round(s * sa * 64) / 64)
            assert abs(y) <= 1
            x = _solve_mag(mask[r, c], T, y, ca)
            if edge == "right":
                p[r, 40] = x
                p[r + 1, 39] = y
            else:
                p[r, 0] = -x
                p[r + 1, 1] = y
        else:
            x = F(np.round(s * ca * 64) / 64)
            assert abs(x) <= 1
            y = _solve_mag(mask[r, c], T, x, sa)
            if edge == "top":
                p[0, c] = -y
                p[1, c + 1] = x
            else:
                p[40, c] = y
                p[39, c + 1] = x
    return p


def bins_patch(bins, T=0.5):
    return site_patch([(bin_angle(b), T if np.isscalar(T) else T[i]) for i, b in enumerate(bins)])


# ---- planted patches --------------------------------------------------------------------------------------------------------------
def _ramps():
    out = []
    for code in range(8):
        xp, yp, big = code & 4, code & 2, code & 1
        for i in range(256):
            if i == 255 and big:
                continue
            small = 255.0 if i == 255 else i + 0.5
            ax, ay = (255.0, small) if big else (small, 255.0)
            xg, yg = (ax if xp else -ax), (ay if yp else -ay)
            out.append(dict(name="ramp/c%d_i%03d" % (code, i), family="ramps", patch=ramp(xg, yg),
                            claim=dict(one_bin=True, entry=(code, i))))
    bx, by = BIG_IDX255
    for code in (1, 3, 5, 7):
        # a gradient pair with |x| > |y| whose quotient rounds to 255: pixel (20, 20) gets (x, y) from two planted neighbours
        # of magnitude below 1, pixel (21, 21) the mirrored (-y, -x); nothing else reaches magnitude 1
        p = np.zeros((PS, PS), F)
        p[20, 21] = bx if code & 4 else -bx
        p[21, 20] = by if code & 2 else -by
        out.append(dict(name="ramp/c%d_i255_rounded" % code, family="ramps", patch=p, claim=dict(entry=(code, 255), nvotes=2)))
    named = [("special_x0_ydown", 0.0, -4.0, dict(one_bin=True, special=True, bin=18)),
             ("x0_yup", 0.0, 4.0, dict(one_bin=True, entry=(2, 0), bin=27)),
             ("angle_pi", -4.0, 2.0 ** -10, dict(one_bin=True, entry=(3, 0), bin=36)),
             ("angle_minus_pi", -4.0, -2.0 ** -10, dict(one_bin=True, entry=(1, 0), bin=0)),
             ("angle_minus_pi_y0", -4.0, 0.0, dict(one_bin=True, entry=(1, 0), bin=0))]
    for name, xg, yg, claim in named:
        out.append(dict(name="ramp/" + name, family="ramps", patch=ramp(xg, yg), claim=claim))
    return out


def single_row_lanes():
    """lanes of the kernel whose 21 consecutive voting-list entries lie in one patch row -> [(lane, row, first column)]"""
    r, c = M.voting_list()
    out = []
    for lane in range(len(r) // 21):
        rr, cc = r[21 * lane:21 * lane + 21], c[21 * lane:21 * lane + 21]
        if (rr == rr[0]).all():
            out.append((lane, int(rr[0]), int(cc[0])))
    return out


def _extremes():
    out = [dict(name="extreme/flat", family="extremes", patch=np.full((PS, PS), 90.0, F), claim=dict(nvotes=0, npeaks={(0, 0.8): 0, (1, 1.0): 0})),
           dict(name="extreme/mag_exactly_1", family="extremes", patch=ramp(1.0, 0.0), claim=dict(nvotes=0, mag=F(1.0))),
           dict(name="extreme/mag_1_plus_ulp", family="extremes", patch=ramp(1.0, 2.0 ** -11),
                claim=dict(one_bin=True, mag=np.nextafter(F(1.0), F(2.0)))),
           dict(name="extreme/mag_rounds_to_1", family="extremes", patch=ramp(1.0, 2.0 ** -13), claim=dict(nvotes=0, mag=F(1.0)))]
    lanes = single_row_lanes()
    for lane, row, col in (lanes[0], lanes[len(lanes) // 2], lanes[-1]):
        xg, yg = np.zeros(PS), np.zeros(PS)
        xg[col:col + 21] = 1.0
        yg[row] = 1.0
        out.append(dict(name="extreme/one_lane_%02d" % lane, family="extremes", patch=separable(xg, yg),
                        claim=dict(lane=lane, nvotes=21, one_bin=True)))
    # rows 12 (yg = +1) and 28 (yg = -1); 1 / 7 / 8 / 9 columns with xg = 1 / 0.75 / -0.75 / -1 and xg = 0 elsewhere (|g| = 1:
    # no vote); every other row has |g| = |xg| <= 1
    xg, yg = np.zeros(PS), np.zeros(PS)
    xg[4:5], xg[6:13], xg[14:22], xg[24:33] = 1.0, 0.75, -0.75, -1.0
    yg[12], yg[28] = 1.0, -1.0
    out.append(dict(name="extreme/counts_1_7_8_9", family="extremes", patch=separable(xg, yg),
                    claim=dict(counts={22: 1, 23: 7, 30: 8, 31: 9, 13: 1, 12: 7, 5: 8, 4: 9})))
    return out


def _peaks():
    out = []

    def add(name, patch, **claim):
        out.append(dict(name="peaks/" + name, family="peaks", patch=patch, claim=claim))

    bump = np.zeros((PS, PS), F)
    bump[20, 20] = 8.0
    # four votes of one weight: left neighbour (+x) bin 18, right (-x, y = 0) bin 0, upper (+y) bin 27, and the lower one has
    # x == 0, y < 0 -- atan2LUTff's special case returns 0, so it joins bin 18 (not bin 9)
    add("centre_bump", bump, counts={0: 1, 18: 2, 27: 1}, equal_weights=True)
    add("tie_two_maxima", bins_patch([5, 23]), tie=(5, 23), npeaks={(0, 1.0): 2, (0, 0.8): 2})
    add("plateau_two_bins", bins_patch([18, 19]), plateau=(18, 19), npeaks={(0, 0.8): 0, (0, 1.0): 0})
    add("peak_bin_0", bins_patch([0]), peak_bins=[0], npeaks={(0, 0.8): 1, (0, 1.0): 1})
    add("peak_bin_35", bins_patch([35]), peak_bins=[35], npeaks={(0, 0.8): 1})
    add("peaks_bins_0_and_29", bins_patch([0, 29]), peak_bins=[0, 29], npeaks={(0, 0.8): 2})
    add("half_differs", bins_patch([2, 20]), npeaks={(0, 0.8): 2, (1, 0.8): 1})
    add("fold_makes_tie", bins_patch([3, 22]), fold_tie=(3, 4), npeaks={(0, 0.8): 2})
    spread = {1: [1], 2: [1, 10], 3: [1, 10, 20], 4: [1, 10, 20, 29], 5: [1, 8, 15, 22, 29]}
    for k, bins in spread.items():
        add("npeaks_%d" % k, bins_patch(bins), npeaks={(0, 0.8): k})
    add("rising_three", bins_patch([2, 11, 20], T=[0.5625, 0.59375, 0.625]), npeaks={(0, 0.8): 3}, rising=True)
    add("alternating18", bins_patch(list(range(0, 36, 2))), npeaks={(0, 0.8): 18, (0, 1.0): 18, (1, 0.8): 9})
    add("alternating18_odd", bins_patch(list(range(1, 36, 2))), npeaks={(0, 0.8): 18})
    return out


def _smooth(a, passes):
    for _ in range(passes):
        a = (np.roll(a, 1, 0) + a + a + np.roll(a, -1, 0)) * F(0.25)
        a = (np.roll(a, 1, 1) + a + a + np.roll(a, -1, 1)) * F(0.25)
    return a.astype(F)


def _random():
    rs = np.random.RandomState(20241)
    out = []
    for i in range(RANDOM_PER_KIND):
        kinds = (("smooth", _smooth(rs.standard_normal((PS, PS)).astype(F) * F(60), 1 + i % 4) + F(20)),
                 ("white", (rs.standard_normal((PS, PS)) * 40).astype(F)),
                 ("lowcontrast", _smooth((rs.standard_normal((PS, PS)) * (1.5 + 0.05 * i)).astype(F), 1) + F(100)),
                 ("integer", np.round(_smooth(rs.standard_normal((PS, PS)).astype(F) * F(90), 2) + F(128))))
        for kind, p in kinds:
            out.append(dict(name="random/%s_%02d" % (kind, i), family="random", patch=np.ascontiguousarray(p, F), claim=dict()))
    return out


def planted():
    """every planted patch, built once: list of dict(name, family, patch, claim)"""
    global _planted
    if _planted is None:
        _planted = _ramps() + _extremes() + _peaks() + _random()
        for c in _planted:
            assert c["patch"].shape == (PS, PS) and c["patch"].dtype == F and np.isfinite(c["patch"]).all(), c["name"]
            c["patch"].setflags(write=False)
    return _planted


def patches():
    return np.stack([c["patch"] for c in planted()])


def family_counts():
    out = {}
    for c in planted():
        out[c["family"]] = out.get(c["family"], 0) + 1
    return out


def region_records(dtype, tuples):
    """region records (oracle.REGION / mods_amd.REGION) of (x, y, s, a11, a12, a21, a22) tuples"""
    t = np.asarray(tuples, np.float64).reshape(-1, 7)
    regs = np.zeros(len(t), dtype)
    for side in ("det_kp", "reproj_kp"):
        for q, f in enumerate(("x", "y", "s", "a11", "a12", "a21", "a22")):
            regs[side][f] = t[:, q]
        regs[side]["response"] = 1.0
        regs[side]["pyramid_scale"] = t[:, 2]
    regs["id"] = np.arange(len(t))
    regs["parent_id"] = np.arange(len(t))
    return regs


MARGIN = 24      # the window's corner test reads +- 21 around the centre


def compose(stack=None):
    """(image f32, centres [n, 2] int (x, y)): every patch in its own 41 x 41 cell of one image, `MARGIN - 20` px of zeros around"""
    stack = patches() if stack is None else np.asarray(stack, F)
    n = len(stack)
    per_row = int(np.ceil(np.sqrt(n)))
    rows = (n + per_row - 1) // per_row
    off = MARGIN - HALF
    img = np.zeros((2 * off + rows * PS, 2 * off + per_row * PS), F)
    centres = np.zeros((n, 2), np.int64)
    for k in range(n):
        r0, c0 = off + (k // per_row) * PS, off + (k % per_row) * PS
        img[r0:r0 + PS, c0:c0 + PS] = stack[k]
        centres[k] = (c0 + HALF, r0 + HALF)
    return img, centres


def identity_regions(dtype, centres):
    c = np.asarray(centres, np.float64)
    return region_records(dtype, np.column_stack([c[:, 0], c[:, 1], np.ones(len(c)), np.ones(len(c)), np.zeros(len(c)),
                                                  np.zeros(len(c)), np.ones(len(c))]))


def expected_records(regs, angles, max_ang=1, upright=0):
    """DetectOrientation's output for regions that all pass the border test, from their angle lists (synth-detection.cpp:
    889-915): one copy per angle with the shape turned by (cosf(-angle), sinf(-angle)) and id 0, then the upright copy"""
    lm = M.libm()
    out = []
    for i in range(len(regs)):
        base = regs[i:i + 1].copy()
        if max_ang > 0:
            base["id"] = 0
            k = base["det_kp"]
            b11, b12, b21, b22 = (float(k[f][0]) for f in ("a11", "a12", "a21", "a22"))
            for a in angles[i]:
                ci, si = float(lm.cosf(-float(a))), float(lm.sinf(-float(a)))
                t = base.copy()
                t["det_kp"]["a11"] = b11 * ci - b12 * si
                t["det_kp"]["a12"] = b11 * si + b12 * ci
                t["det_kp"]["a21"] = b21 * ci - b22 * si
                t["det_kp"]["a22"] = b21 * si + b22 * ci
                out.append(t)
        if upright:
            out.append(base)
    return np.concatenate(out) if out else regs[:0].copy()


_analysis = None


def analysis(oracle):
    """orient_model.analyse of every planted patch, computed once per process and shared by the tests"""
    global _analysis
    if _analysis is None:
        _analysis = M.analyse(oracle, patches())
    return _analysis


def counts_per_centre(recs, centres):
    """records per centre (x, y): how many angles each region of `centres` got"""
    key = {(float(x), float(y)): i for i, (x, y) in enumerate(centres)}
    n = np.zeros(len(centres), np.int64)
    for x, y in zip(recs["det_kp"]["x"].tolist(), recs["det_kp"]["y"].tolist()):
        n[key[(x, y)]] += 1
    return n


# ---- geometric cases ----------------------------------------------------------------------------------------------------------------
GEO_ROWS, GEO_COLS = 200, 260


def textured_image():
    rs = np.random.RandomState(977)
    a = _smooth((rs.standard_normal((GEO_ROWS, GEO_COLS)) * 160).astype(F), 3)
    return np.ascontiguousarray(a + F(15), F)         # blurred noise around 15: about a third of the pixels are negative


def small_image():
    rs = np.random.RandomState(978)
    return np.ascontiguousarray(_smooth((rs.standard_normal((30, 30)) * 120).astype(F), 2) + F(10), F)


def _rot(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return (c, -s, s, c)


ISO = (1.0, 0.0, 0.0, 1.0)
SHEAR = (1.0, 0.8, 0.0, 1.0)
ANISO = (5.0 ** 0.5, 0.0, 0.0, 5.0 ** -0.5)                    # 5 : 1, determinant 1
ANISO_ROT = (1.9365, -1.1180, 0.2236, 0.3873)                   # the same turned by 30 degrees (rounded entries)
NEGDET = (1.0, 0.0, 0.0, -1.0)
NEARZERO = (1e-6, 0.0, 0.0, 1e-6)

# (name, (x, y, s, a11, a12, a21, a22), {mr_size: claimed class}); every region runs at every mr_size of MR_SIZES
GEOMETRIC = [
    ("iso_s1_centre", (130.3, 100.6, 1.0) + ISO, {1.0: "inside", 5.1962: "inside", 8.0: "inside", 20.0: "inside"}),
    ("iso_s4_centre", (130.3, 100.6, 4.0) + ISO, {5.1962: "inside", 20.0: "inside"}),
    ("iso_s4p7_touch", (130.0, 100.0, 4.7) + ISO, {20.0: "touch_inside", 8.0: "inside"}),
    ("rot30_s2", (97.25, 88.5, 2.0) + _rot(30.0), {20.0: "inside", 1.0: "inside"}),
    ("rot200_s3p6_frac", (140.125, 101.875, 3.6) + _rot(200.0), {20.0: "touch_inside", 8.0: "inside"}),
    ("shear_s2", (120.5, 100.5, 2.0) + SHEAR, {20.0: "inside", 5.1962: "inside"}),
    ("aniso_s1p5", (131.0, 99.0, 1.5) + ANISO, {20.0: "inside", 8.0: "inside"}),
    ("aniso_rot_s2", (131.7, 99.2, 2.0) + ANISO_ROT, {20.0: "touch_inside", 5.1962: "inside"}),
    ("negdet_s2", (88.4, 120.9, 2.0) + NEGDET, {20.0: "inside", 5.1962: "inside"}),
    ("nearzero", (50.5, 60.25, 1.0) + NEARZERO, {20.0: "inside", 1.0: "inside"}),
    ("over_left", (20.0, 100.0, 3.0) + ISO, {20.0: "overhang", 8.0: "overhang", 5.1962: "inside", 1.0: "inside"}),
    ("over_right", (239.5, 100.0, 3.0) + ISO, {20.0: "overhang", 8.0: "overhang"}),
    ("over_top", (130.0, 19.25, 3.0) + ISO, {20.0: "overhang", 8.0: "overhang"}),
    ("over_bottom", (130.0, 180.5, 3.0) + ISO, {20.0: "overhang", 8.0: "overhang", 5.1962: "touch_inside"}),
    ("over_corner", (20.0, 19.5, 3.0) + ISO, {20.0: "overhang", 8.0: "overhang"}),
    ("over_corner_rot", (230.0, 170.0, 3.0) + _rot(45.0), {20.0: "overhang"}),
    ("over_aniso", (40.0, 100.0, 2.0) + ANISO, {20.0: "overhang"}),
    ("drop_left", (12.0, 100.0, 3.0) + ISO, {m: "dropped" for m in MR_SIZES}),
    ("drop_bottom", (130.0, 190.0, 3.0) + ISO, {m: "dropped" for m in MR_SIZES}),
    ("drop_big", (130.0, 100.0, 20.0) + ISO, {m: "dropped" for m in MR_SIZES}),
]
# the 30 x 30 image: the K_SIGMA box of s = 1 is 10 px, the window at mr_size 20 is 41 px
SMALL_GEOMETRIC = [
    ("small_centre", (15.0, 15.0, 1.0) + ISO, {20.0: "overhang", 8.0: "inside", 1.0: "inside"}),
    ("small_offcentre_rot", (13.5, 16.25, 1.0) + _rot(25.0), {20.0: "overhang", 8.0: "touch_inside"}),
    ("small_dropped", (4.0, 15.0, 1.0) + ISO, {20.0: "dropped"}),
]


def geometric_regions(dtype, cases=None):
    return region_records(dtype, [c[1] for c in (GEOMETRIC if cases is None else cases)])


def patch_scale(mr_size):
    return float(2 * int(mr_size) + 1) / 41.0


def tap_coordinates(reg, mr_size):
    """the f32 sample coordinates of interpolate() for one region tuple: running sums along rows and columns -> (WX, WY) [41, 41]"""
    x, y, s, a11, a12, a21, a22 = reg
    sc = F(patch_scale(mr_size) * s)
    a11, a12, a21, a22 = (F(F(v) * sc) for v in (a11, a12, a21, a22))
    rx, ry = F(x) - F(HALF) * a12, F(y) - F(HALF) * a22
    WX, WY = np.zeros((PS, PS), F), np.zeros((PS, PS), F)
    for j in range(PS):
        wx, wy = rx - F(HALF) * a11, ry - F(HALF) * a21
        for i in range(PS):
            WX[j, i], WY[j, i] = wx, wy
            wx, wy = F(wx + a11), F(wy + a21)
        rx, ry = F(rx + a12), F(ry + a22)
    return WX, WY


def taps_outside(reg, mr_size, rows, cols):
    """taps the bounds branch of interpolate() sets to 0"""
    WX, WY = tap_coordinates(reg, mr_size)
    inside = (WX >= 0) & (WY >= 0) & (np.floor(WX) < cols - 1) & (np.floor(WY) < rows - 1)
    return int((~inside).sum())


def border_tuples(reg, mr_size, rows, cols):
    """(box tuple, window tuple) for check_borders: the K_SIGMA box on the unscaled shape, the 41-tap window on the scaled one"""
    x, y, s, a11, a12, a21, a22 = reg
    sc = F(patch_scale(mr_size) * s)
    box = (cols, rows, x, y, a11, a12, a21, a22, int(K_SIGMA * s))
    win = (cols, rows, x, y) + tuple(float(F(F(v) * sc)) for v in (a11, a12, a21, a22)) + (PS,)
    return box, win
