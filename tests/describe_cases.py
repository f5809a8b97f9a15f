"""The inputs of the describe-path tests (tests/test_describe_cases_cpu.py, tests/test_describe_plan_cpu.py,
tests/test_gpu_describe_paths.py, tests/test_gpu_describe_chunks.py, tests/describe_chunk_child.py), built once per process and
left alone.

Image: 240x320 f32 with full mantissas (a smooth term plus uniform noise that is not floored, clipped to [0, 255]).  The floored
synthetic images make many of the describe stage's sums exact; this one does not.

Window sizes: a region with scale s described at mr_size = 1.0 gets the window P = 2 * ceil(s) + 3, so s = (P - 3) / 2 picks P
exactly.  SIZES holds every odd P of 19..135 and, above that, the smallest P of every distinct (rows per LDS row tile, columns per
LDS column tile, last row tile ragged or not) that the planner of the description stage (mods_amd/csrc/describe_plan.cpp) plans
today, plus both sides of every path boundary: 33|35 (fused column filter | separate), 43|45 (whole-window row tile | clamp to 32
rows), 65|67 (column-filter stride 64, one tile | stride 96, several tiles), 471|473 (LDS column filter | global-memory one),
983|985 (fused sampling kernel | k_patch_sample + global row filter), 1023|1025 (the 128-column tile edge of k_patch_sample), 2329
(the last size accepted; 2331 is refused).  Which path a size takes is READ from the library, never restated here: on the CPU from
the planner alone (mods_amd.describe_plan, tests/test_describe_plan_cpu.py), on the GPU from what the device call booked
(Context.describe_counters()), and the GPU tests assert that the two agree.  class_of() names the path of a per-window signature.

Regions per P (three, in this order): interior -- the whole P x P window samples inside the image, the no-border path; top-left and
bottom-right -- most of the window lies outside, the border path.
"""
import functools
import math

import numpy as np

ROWS, COLS = 240, 320
MR_SIZE = 1.0
DENSE = tuple(range(19, 137, 2))
SPARSE = (139, 141, 143, 145, 147, 149, 153, 159, 161, 163, 165, 167, 171, 179, 181, 185, 187, 193, 195, 199, 201, 205, 207, 213,
          217, 219, 225, 227, 235, 237, 247, 249, 253, 259, 263, 267, 273, 281, 283, 299, 307, 327, 329, 335, 353, 355, 381, 385,
          391, 395, 417, 427, 471, 473, 493, 495, 657, 983, 985, 1023, 1025, 2083, 2329)
SIZES = DENSE + SPARSE
REFUSED_P = 2331                   # the blur kernel of this window has 513 taps
DIRECT_S = 7.0                     # patchImageSize 15: 15 / 41 <= 0.4, the direct branch; s = 8 gives P = 19
CENTRES = ((160.3, 120.7), (1.5, 2.25), (COLS - 2.5, ROWS - 1.75),     # interior, top-left, bottom-right: the regions of the sweep
           (60.75, 180.4), (250.1, 40.9))                              # two more for the calls of five regions
# the parametrised groups of tests/test_gpu_describe_paths.py: each a few seconds of oracle time at the most
GROUPS = (("p19_65", tuple(p for p in SIZES if p <= 65)), ("p67_135", tuple(p for p in SIZES if 67 <= p <= 135)),
          ("p139_207", tuple(p for p in SIZES if 139 <= p <= 207)), ("p213_299", tuple(p for p in SIZES if 213 <= p <= 299)),
          ("p307_495", tuple(p for p in SIZES if 307 <= p <= 495)), ("p657_1025", tuple(p for p in SIZES if 657 <= p <= 1025)),
          ("p2083", (2083,)), ("p2329", (2329,)))
assert tuple(p for _, g in GROUPS for p in g) == SIZES
ARENA_FLOOR_FLOATS = 16 << 18      # MODSX_ARENA_MB = 16, the smallest arena describe_batch accepts

# the path classes of the planner, in the order of P in which they occur, and what the sweep over SIZES must show
CLASSES = ("fused", "whole_window_row_tile", "clamp_32_rows", "row_tiles_le_32", "several_col_tiles", "lds_rows_global_cols", "all_global")
CLASS_SIZE = dict(zip(CLASSES, (25, 39, 47, 63, 77, 493, 985)))        # the size of each class that gets the extra calls
ROW_TILE_VALUES = 47        # distinct LDS row tiles per window over SIZES (1 .. 492), as the counters gave them on an MI355X and as
                            # the planner alone gives them on a CPU (tests/test_describe_plan_cpu.py)
COL_TILE_VALUES = 15        # distinct LDS column tiles per window over SIZES (1 .. 41): every value the planner can give
PER_WINDOW = ("fused_windows", "clamped_windows", "lds_row_tiles", "lds_col_tiles", "sample_tiles", "global_row_tiles", "global_col_tiles")
# the counters that add up over calls (max_chunks is a running maximum): a device call's difference of two readings equals the
# planner's counters of the same call in these
SUMMED = ("calls", "chunks", "chunks_mid_image", "chunks_later_image", "jobs", "direct_jobs") + PER_WINDOW


def class_of(sig):
    """the path class of a per-window signature {counter of PER_WINDOW: value for one window}"""
    fused, clamped, rt, ct, st, gr, gc = (sig[k] for k in PER_WINDOW)
    if fused:
        assert (rt, ct, st, gr, gc) == (1, 0, 0, 0, 0), sig
        return "fused"
    if st:
        assert rt == 0 and ct == 0 and gr > 0 and gc > 0, sig
        return "all_global"
    assert rt > 0 and gr == 0, sig
    if gc:
        assert ct == 0, sig
        return "lds_rows_global_cols"
    assert ct > 0, sig
    if ct > 1:
        return "several_col_tiles"
    if rt == 1:
        return "whole_window_row_tile"
    return "clamp_32_rows" if clamped else "row_tiles_le_32"


def arena_floats():
    """the window arena of this process, as describe_batch reads it: MODSX_ARENA_MB (at least 16) or 192 MiB, in floats"""
    import os
    mb = os.environ.get("MODSX_ARENA_MB")
    return max(192 if mb is None else int(mb or 0), 16) << 18


@functools.lru_cache(maxsize=None)
def image():
    rng = np.random.default_rng(20240611)
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    smooth = 128.0 + 70.0 * np.sin(x / 17.0 + 0.3) * np.cos(y / 23.0 - 0.2) + 30.0 * np.sin((x + 2.0 * y) / 41.0)
    img = np.clip(smooth + rng.uniform(-45.0, 45.0, (ROWS, COLS)), 0.0, 255.0).astype(np.float32)
    img.setflags(write=False)
    return img


def theta_of(P):
    """rotation of the shape: varies with P, within +-0.6 rad so that the interior window of every P stays inside the 240 rows"""
    return ((P * 37) % 101) / 100.0 * 1.2 - 0.6


def shape_of(P, interior):
    """A = R(theta) * diag(1.4, 0.7), times min(1, 160 / P) for the interior region"""
    t = theta_of(P)
    k = min(1.0, 160.0 / P) if interior else 1.0
    c, s = math.cos(t), math.sin(t)
    return (1.4 * c * k, -0.7 * s * k, 1.4 * s * k, 0.7 * c * k)


@functools.lru_cache(maxsize=None)
def _template():
    """a valid REGION record: one keypoint through the oracle's DetectAffineRegions"""
    from oracle import pyoracle as O
    kp = np.zeros(1, O.KEYPOINT)
    kp["x"], kp["y"], kp["s"], kp["a11"], kp["a22"], kp["response"], kp["pyramid_scale"] = 10.0, 10.0, 3.0, 1.0, 1.0, 1.0, 1.0
    r = O.detect_affine_regions(kp)
    r["reproj_kp"] = r["det_kp"]
    return r


def make_regions(specs):
    """specs: (x, y, (a11, a12, a21, a22), s) -> REGION records with det_kp and reproj_kp both set"""
    out = np.repeat(_template(), len(specs))
    for i, (x, y, A, s) in enumerate(specs):
        for kp in ("det_kp", "reproj_kp"):
            k = out[kp]
            k["x"][i], k["y"][i], k["s"][i] = x, y, s
            k["a11"][i], k["a12"][i], k["a21"][i], k["a22"][i] = A
        out["id"][i] = i
    return out


def s_of(P):
    return (P - 3) / 2.0


def window_of(s, mr_size=MR_SIZE):
    """DescribeRegions' window of a region: P of the smoothed branch, 0 for the direct branch (synth-detection.hpp:186-224)"""
    pis = 2 * int(np.float32(math.ceil(s * mr_size))) + 1
    return pis + 2 if np.float32(pis) / np.float32(41) > 0.4 else 0


def regions_of(P, which=(0, 1, 2)):
    """the regions of window size P: interior, top-left, bottom-right (P = 0: the direct branch, s = DIRECT_S)"""
    s = s_of(P) if P else DIRECT_S
    Pa = P if P else 19
    return make_regions([(CENTRES[w][0], CENTRES[w][1], shape_of(Pa, w == 0), s) for w in which])


def interior_corners(P):
    """the four corners interpolate()'s border test looks at for the interior region of P (half extent ceil(P / 2), f32 as there)"""
    f = np.float32
    a11, a12, a21, a22 = (f(v) for v in shape_of(P, True))
    cx, cy, h = f(CENTRES[0][0]), f(CENTRES[0][1]), f(math.ceil(P / 2.0))
    return [(float(cx + sx * h * a11 + sy * h * a12), float(cy + sx * h * a21 + sy * h * a22)) for sx in (-1, 1) for sy in (-1, 1)]


_REFS = {}


def oracle_rows(jobs, threads=8):
    """[oracle.describe_regions(image(), regs, **kw) for regs, kw in jobs], region by region on a thread pool (ctypes releases the
    GIL; the oracle describes every region on its own, so the rows of a list are the rows of its regions)"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import pyoracle as O
    img = image()
    flat = [(j, i) for j, (regs, _) in enumerate(jobs) for i in range(len(regs))]
    flat.sort(key=lambda ji: -float(jobs[ji[0]][0]["det_kp"]["s"][ji[1]]))          # the large windows first
    out = [np.zeros((len(regs), 128), np.float32) for regs, _ in jobs]

    def one(ji):
        j, i = ji
        out[j][i] = O.describe_regions(img, jobs[j][0][i:i + 1], **jobs[j][1])[0]

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, flat))
    for o in out:
        o.setflags(write=False)
    return out


def references(sizes=None):
    """{P: oracle descriptors of regions_of(P)} for `sizes` (default: SIZES and 0, the direct branch), RootSIFT with photometric
    normalisation; computed once per process and size"""
    sizes = tuple(SIZES + (0,)) if sizes is None else tuple(sizes)
    todo = [P for P in sizes if P not in _REFS]
    for P, d in zip(todo, oracle_rows([(regions_of(P), dict(mr_size=MR_SIZE)) for P in todo])):
        _REFS[P] = d
    return {P: _REFS[P] for P in sizes}


# ---------------- the chunk cases (tests/describe_chunk_child.py) -----------------------------------------------------------------
VIEW_TILTS = (1.0, 2.0, 4.0, 6.0, 8.0)     # TiltSet of the views case: 11 views
VIEWS_DESC_MR = 24.0
CRAFTED_RUNS = ((315, 60), (2083, 1), (0, 20), (315, 60))      # (P, regions) of the crafted single image, in list order


_VIEWS = []


def views_case(oracle, small_a):
    """(regions, descriptors) of the views case from the oracle: image 0 of the small pair under VIEW_TILTS with desc_mrSize =
    VIEWS_DESC_MR; computed once per process (small_a is the session's small pair, always the same image)"""
    if not _VIEWS:
        regs, desc = oracle.detect_describe_views(small_a, oracle.set_vs_pars([1.0], list(VIEW_TILTS), 360.0, 0.5, 1, []),
                                                  desc=(VIEWS_DESC_MR, 41, 0, 1, 1, 0.2), threads=8)
        for a in (regs, desc):
            a.setflags(write=False)
        _VIEWS.append((regs, desc))
    return _VIEWS[0]


@functools.lru_cache(maxsize=None)
def crafted_regions():
    """60 regions of P = 315, one of P = 2083 (larger than the 16 MiB arena: it must travel alone), 20 direct-branch regions,
    60 of P = 315; centres on a lattice over the image, shapes turning from region to region"""
    specs = []
    for P, cnt in CRAFTED_RUNS:
        for _ in range(cnt):
            i = len(specs)
            t = 0.37 * i
            k = 0.9 + 0.004 * i
            A = (1.1 * k * math.cos(t), -0.8 * k * math.sin(t), 1.1 * k * math.sin(t), 0.8 * k * math.cos(t))
            if P == 0:
                A = tuple(2.0 * v for v in A)
            specs.append((20.25 + (i * 53) % 280, 15.5 + (i * 31) % 210, A, s_of(P) if P else DIRECT_S))
    r = make_regions(specs)
    r.setflags(write=False)
    return r


def greedy_cuts(windows, arena=ARENA_FLOOR_FLOATS):
    """first region of every chunk after the first: the planner closes a chunk before the region whose P * P floats would
    overflow the arena, unless the chunk is still empty (an independent restatement of the rule: the planner itself,
    mods_amd.describe_plan, is checked against it in tests/test_describe_plan_cpu.py)"""
    cuts, used, count = [], 0, 0
    for i, P in enumerate(windows):
        need = P * P
        if P > 0 and used + need > arena and count:
            cuts.append(i)
            used, count = 0, 0
        used += need
        count += 1
    return cuts
