"""Inputs of the pyramid parity suite: blur shapes, the tile-height boundary, a mixed batch, planted response planes for the
extrema scan and a batch that fills the scan's job table.  tests/test_pyramid_cases_cpu.py proves from the oracle and
mods_amd.blur_geometry that they reach what tests/test_gpu_pyramid.py relies on; the GPU module only compares.

Everything here is numpy on fixed seeds (RandomState, whose streams are frozen), so the inputs are the same everywhere.
"""
import numpy as np

# ---- blur ---------------------------------------------------------------------------------------------------------------------
# one sigma per instantiated half width R = 1 .. 8 of k_blur_hess (ksize = 2 R + 1); 2.6 is also the switch's default label
BLUR_SIGMAS = (0.4, 0.7, 1.0, 1.2263, 1.5199, 1.9466, 2.4525, 2.6)
BLUR_KSIZES = (3, 5, 7, 9, 11, 13, 15, 17)
REFUSED_SIGMA = 2.84          # ksize 19: more taps than the pyramid kernels hold
# around the 64-column tile and the 16-row tile; 2 x 2 is smaller than every halo
BLUR_COLS = (2, 63, 64, 65, 129)
BLUR_ROWS = (2, 15, 16, 17, 33)
# 257 columns are 5 tile columns: 16353 rows are 512 tile rows of 32 (2560 tiles, the first launch on 32-row tiles),
# 16321 rows are 511 (2555 tiles: 16-row tiles)
TILE32_SHAPE = (16353, 257)
TILE16_SHAPE = (16321, 257)
TILE_BOUNDARY = 2560
# the half widths the levels of an octave never use (numberOfScales = 3: R = 4 .. 7) are sent over 32-row tiles by a plain blur
TILE32_BLUR_SIGMAS = (0.4, 0.7, 1.0, 2.6)
TILE16_BLUR_SIGMAS = (0.4, 2.6)


def image(rows, cols, seed):
    """integers 0 .. 255 as f32: a slow wave under uniform noise"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    img = 128 + 60 * np.sin(x / 7.0) * np.cos(y / 5.0) + rs.uniform(-30, 30, (rows, cols))
    return np.clip(np.floor(img), 0, 255).astype(np.float32)


def octave_shapes(rows, cols, border):
    """the octave rule of detectPyramidKeypoints (pyramid.cpp:540-573): halve with cvRound (round half to even, as Python's
    round) while both sides exceed 2 border + 2"""
    out = []
    while rows > 2 * border + 2 and cols > 2 * border + 2 and len(out) < 24:
        out.append((rows, cols))
        rows, cols = int(round(rows * 0.5)), int(round(cols * 0.5))
    return out


def tiles(shapes, th):
    return sum(((c + 63) // 64) * ((r + th - 1) // th) for r, c in shapes)


# ---- mixed batch ----------------------------------------------------------------------------------------------------------------
# 65 columns: the second tile column of every image holds one pixel.  Octave 0 has 2 x (512 + 501 + 269 + 2) = 2568 32-row tiles;
# the last image has two octaves where the others have three (default border 5)
MIXED_SHAPES = ((16383, 65), (16001, 65), (8601, 65), (40, 65))


def mixed_batch():
    return [image(r, c, 40 + i) for i, (r, c) in enumerate(MIXED_SHAPES)]


# ---- the job-table flush ----------------------------------------------------------------------------------------------------------
# 32 images of seven octaves at border 1, numberOfScales = 6: 32 x 7 x 6 = 1344 (image, octave, level) jobs > NMS_MAXJ = 1024.
# The scan collects octave after octave, so the launch after the flush holds the last 22 images' octave 5 and everyone's octave 6
NMS_MAXJ = 1024
FLUSH_PARAMS = dict(numberOfScales=6, border=1, mode=4)
FLUSH_SHAPES = tuple((320 + (i % 7), 329 - (i % 5)) for i in range(32))


def flush_batch():
    rs = np.random.RandomState(77)
    return [np.floor(rs.uniform(0, 256, s)).astype(np.float32) for s in FLUSH_SHAPES]


def flush_jobs():
    """(jobs of the batch, jobs in the launches before the last) by the rule of scan_extrema: octave-major over the images that
    have the octave, numberOfScales jobs per entry, a launch as soon as the next entry would not fit"""
    S, B = FLUSH_PARAMS["numberOfScales"], FLUSH_PARAMS["border"]
    octs = [octave_shapes(r, c, B) for r, c in FLUSH_SHAPES]
    total = held = flushed = 0
    for o in range(max(len(x) for x in octs)):
        for x in octs:
            if len(x) <= o or x[o][0] - 2 * B <= 0 or x[o][1] - 2 * B <= 0:
                continue
            if held + S > NMS_MAXJ:
                flushed += held
                held = 0
            held += S
            total += S
    return total, flushed


# ---- planted response planes --------------------------------------------------------------------------------------------------------
def mean7x(a):
    """7-point mean along the columns (replicated ends)"""
    p = np.pad(a, ((0, 0), (0, 0), (3, 3)), mode="edge")
    return sum(p[:, :, k:k + a.shape[2]] for k in range(7)) / 7.0


def box3(a):
    """3 x 3 mean inside every plane: smooth in both directions, so the Newton walk leaves its pixel more often"""
    p = np.pad(a, ((0, 0), (1, 1), (1, 1)), mode="edge")
    return sum(p[:, i:i + a.shape[1], j:j + a.shape[2]] for i in range(3) for j in range(3)) / 9.0


def noise_planes(L, rows, cols, seed, smooth=mean7x):
    rs = np.random.RandomState(seed)
    resp = (smooth(rs.standard_normal((L, rows, cols))) * 100).astype(np.float32)
    blur = rs.uniform(0, 255, (L, rows, cols)).astype(np.float32)
    return resp, blur


NAN_BLOCK = (slice(None), slice(12, 18), slice(20, 26))   # a constant 6 x 6 x 5 block above the threshold
EQUAL_PAIRS = (((1, 30, 40), (1, 30, 41), 60.0), ((2, 8, 60), (2, 9, 60), 45.0),      # (level, row, column) twice, value
               ((3, 25, 10), (3, 25, 11), -60.0), ((2, 33, 70), (2, 34, 70), -45.0))


def plateau_planes():
    """zeros with a constant block (solve3 divides 0 by 0: the NaN exit) and pairs of equal neighbours, of both signs, each of
    which is a 3x3x3 extremum (the tests are `>` and `<`)"""
    resp = np.zeros((5, 40, 80), np.float32)
    resp[NAN_BLOCK] = 50.0
    for a, b, v in EQUAL_PAIRS:
        resp[a] = resp[b] = v
    blur = np.random.RandomState(5).uniform(0, 255, resp.shape).astype(np.float32)
    return resp, blur


class ScanCase(object):
    def __init__(self, name, planes, **params):
        self.name, self._planes, self.params = name, planes, params
        self.L = params.get("numberOfScales", 3) + 2
        self.border = params.get("border", 5)

    def planes(self):
        resp, blur = self._planes()
        assert resp.shape[0] == self.L and resp.dtype == np.float32 and blur.dtype == np.float32
        return resp, blur

    def __repr__(self):
        return self.name


# scan windows of width 1, 64, 65, 129 and height 1, 16, 17, 33 at the default border 5 (mode 4: every extremum counts)
WINDOW_SHAPES = {(11, 11): 18, (26, 74): 1, (27, 75): 1, (43, 139): 1, (11, 139): 1, (43, 11): 1}   # shape -> seed
BIG = "noise5"          # more than 1024 accepted extrema: the fresh-context case

SCAN_CASES = [
    ScanCase("noise5", lambda: noise_planes(5, 120, 330, 2)),
    ScanCase("noise5_mode4", lambda: noise_planes(5, 120, 330, 2), mode=4),
    ScanCase("noise8", lambda: noise_planes(8, 60, 200, 2), numberOfScales=6),
    ScanCase("border1", lambda: noise_planes(5, 48, 80, 122, box3), border=1),
    ScanCase("border2", lambda: noise_planes(5, 48, 80, 45, box3), border=2),
    ScanCase("plateau", plateau_planes),
] + [ScanCase("window_%dx%d" % (r - 10, c - 10), (lambda r=r, c=c, s=s: noise_planes(5, r, c, s)), mode=4)
     for (r, c), s in WINDOW_SHAPES.items()]


def scan_case(name):
    return [c for c in SCAN_CASES if c.name == name][0]


def oracle_scan(O, case):
    """the oracle's answers for a case: the report without the claim (every localised extremum), the keypoints and the report with it"""
    resp, blur = case.planes()
    p = O.default_params(**case.params)
    _, rep = O.scan_levels(resp, blur, p, claim=False)
    kp, rep_claim = O.scan_levels(resp, blur, p, claim=True)
    return dict(report=rep, accepted=rep[rep["exit"] == 0], kp=kp, report_claim=rep_claim)


CAND_FIELDS = ("level", "r0", "c0", "r", "c", "type")
SSKP_FIELDS = ("octave", "level", "r0", "c0", "r", "c", "type", "b0", "b1", "b2", "val", "x", "y", "s", "pixelDistance")


def scan_mismatches(cands, kp, ref):
    """what differs between the device's answer for a case (raw accepted candidates in any order, keypoints after order and claim)
    and oracle_scan's: a list of strings, empty when everything is equal.  Floats are compared as bits."""
    bad = []
    acc = ref["accepted"]
    if len(cands) != len(acc):
        return ["%d accepted candidates, the oracle has %d" % (len(cands), len(acc))]
    if len(cands):
        if (cands["img"] != 0).any() or (cands["octave"] != 0).any():
            bad.append("image / octave of a candidate is not 0")
        c = cands[np.lexsort((cands["c0"], cands["r0"], cands["level"]))]      # the oracle's scan order
        for f in CAND_FIELDS:
            if not np.array_equal(c[f], acc[f]):
                bad.append("candidate field " + f)
        for f in ("b0", "b1", "b2", "val"):
            if not np.array_equal(c[f].view(np.uint32), acc[f].view(np.uint32)):
                bad.append("candidate field %s (bits)" % f)
    if len(kp) != len(ref["kp"]):
        return bad + ["%d keypoints after the claim, the oracle has %d" % (len(kp), len(ref["kp"]))]
    for f in SSKP_FIELDS:
        a, b = kp[f], ref["kp"][f]
        same = np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)
        if not same:
            bad.append("keypoint field " + f)
    return bad


def run_scan_case(ctx, modsx, case, ref, per_level=False):
    """debug_scan_levels on a case -> the list of mismatches with oracle_scan's `ref`, the path the counters show included.
    per_level: the process runs with MODSX_NMS_PER_LEVEL, so L = 5 takes the per-level kernel as well."""
    resp, blur = case.planes()
    S = case.L - 2
    before = ctx.detect_counters()
    cands, kp = ctx.debug_scan_levels(resp, blur, modsx.default_hessaff_params(**case.params))
    after = ctx.detect_counters()
    d = {k: after[k] - before[k] for k in after}
    bad = scan_mismatches(cands, kp, ref)
    octave_kernel = S == 3 and not per_level
    w, h = resp.shape[2] - 2 * case.border, resp.shape[1] - 2 * case.border
    t = ((w + 63) // 64) * ((h + 15) // 16)
    want = dict(scan_per_octave=int(octave_kernel), scan_per_level=int(not octave_kernel), nms_flushes=0)
    for k, v in want.items():
        if d[k] != v:
            bad.append("counter %s moved by %d, expected %d" % (k, d[k], v))
    for k, v in dict(last_jobs=S, last_tiles=t if octave_kernel else t * S, last_accepted=len(ref["accepted"])).items():
        if after[k] != v:
            bad.append("counter %s reads %d, expected %d" % (k, after[k], v))
    for k in d:
        if k.startswith("blur_") or k in ("hessian", "resize"):
            if d[k]:
                bad.append("counter %s moved in a scan" % k)
    return bad
