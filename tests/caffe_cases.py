"""The inputs of the learned-descriptor front end's tests (tests/test_caffe_model_cpu.py, test_host_abi_caffe.py,
test_gpu_caffe.py): two planted colour images and their gray forms, a region list that reaches every path of interpolate, and
rows for the three norms.  Expected values never come from here: tests/caffe_model.py computes them."""
import functools

import numpy as np

import caffe_model as M
from mods_amd import REGION

IMAGES = {"a": (48, 64), "b": (29, 37)}            # name -> (rows, cols)
PATCH_SIZES = (1, 3, 41, 63, 65, 127, 129, 255)    # both sides of one and two wavefronts of rows, and the maximum
ALL_COUNTS_AT = (41, 65)                           # the patch sizes at which every region count runs
COUNTS = (0, 1, 2, 3, 63, 64, 65)
MEANS = ((104.0, 117.0, 123.0), (104.9, -3.7, 0.5), (0.0, 0.0, 0.0))
MR_SIZE = 3.0 * 3.0 ** 0.5                         # PatchExtractionParams: patchImageSize = 11

NORM_WIDTHS = (1, 3, 4, 63, 64, 65, 128, 256, 4096)
NORM_ROW_COUNTS = (1, 63, 64, 65, 257)
NORMS = (M.NORM_L2, M.NORM_L1, M.NORM_ROOTL2)
NORM_NAMES = {M.NORM_L2: "l2", M.NORM_L1: "l1", M.NORM_ROOTL2: "root"}


@functools.lru_cache(None)
def planes(name):
    """(B, G, R) f32 [rows][cols].  B holds consecutive integers along a row (x + 2 y): a half-pixel offset samples k + 0.5
    exactly.  G is noise that leaves 0 .. 255 on both sides (-20 and 300 among its values).  R is smooth and fractional."""
    rows, cols = IMAGES[name]
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    rng = np.random.RandomState(11 + rows)
    B = (x + 2 * y).astype(np.float32)
    G = rng.uniform(-20.0, 300.0, (rows, cols)).astype(np.float32)
    G[0, 0], G[1, 1], G[-1, -1], G[-2, -2] = -20.0, 300.0, 300.0, -20.0
    R = (127.0 + 120.0 * np.sin(0.37 * x) * np.cos(0.23 * y) + 0.25).astype(np.float32)
    for p in (B, G, R):
        p.setflags(write=False)
    return B, G, R


@functools.lru_cache(None)
def gray(name):
    B, G, R = planes(name)
    g = ((B + G + R) / np.float32(3)).astype(np.float32)
    g[0, 0], g[-1, -1] = -20.0, 300.0
    g.setflags(write=False)
    return g


def region(x, y, s, a11=1.0, a12=0.0, a21=0.0, a22=1.0):
    r = np.zeros(1, REGION)
    for f in ("x", "y", "a11", "a12", "a21", "a22", "s", "response", "pyramid_scale"):
        r["det_kp"][f] = 1e9            # only reproj_kp is read
    k = r["reproj_kp"]
    k["x"], k["y"], k["s"], k["a11"], k["a12"], k["a21"], k["a22"] = x, y, s, a11, a12, a21, a22
    return r


REGION_NAMES = ("inside", "inside_small", "left", "right", "top", "bottom", "corner", "far_corner", "outside", "rotated",
                "sheared", "anisotropic", "mirrored", "tie", "larger_than_image")


def regions(name, P, mr_size=MR_SIZE):
    """the full list for one image and patch size, in the order of REGION_NAMES.  The footprint of a patch in the image is
    patchImageSize * s pixels whatever P is; only the tie region's scale depends on P (curr_sc = 1: a window of P pixels)."""
    rows, cols = IMAGES[name]
    pis = 2 * int(mr_size) + 1
    cx, cy = cols / 2.0 + 0.3, rows / 2.0 - 0.2
    c30, s30 = np.cos(np.pi / 6), np.sin(np.pi / 6)
    rs = [
        region(cx, cy, 1.0),                                   # well inside: the truncation branch
        region(cx - 1.6, cy + 0.7, 0.31),
        region(3.2, cy, 1.0), region(cols - 4.1, cy, 1.0), region(cx, 3.4, 1.0), region(cx, rows - 3.7, 1.0),
        region(1.5, 1.2, 1.5),                                 # hangs over the corner at (0, 0), where G is -20 and 300
        region(cols - 2.5, rows - 2.2, 0.7),
        region(-100.0, -80.0, 1.0),                            # entirely outside: the blob is -mean
        region(cx, cy, 0.9, c30, -s30, s30, c30),
        region(cx, cy, 0.8, 1.0, 0.6, 0.0, 1.0),
        region(cx, cy, 0.6, 2.0, 0.0, 0.0, 0.5),
        region(cx, cy, 0.9, -1.0, 0.0, 0.0, 1.0),
        region(cols // 2 + 0.5, float(rows // 2), float(P) / float(pis)),      # identity at a half-pixel offset, curr_sc = 1
        region(cx, cy, 20.0),                                  # the window is larger than the image
    ]
    r = np.concatenate(rs)
    r["id"] = np.arange(len(r))
    assert len(r) == len(REGION_NAMES)
    return r


def take(regs, n):
    """n regions: the list, repeated from its start when n is longer"""
    return regs[np.arange(n) % len(regs)].copy()


@functools.lru_cache(None)
def model_bytes(name, colour, P):
    """(u8 [n][3][P][P], border [n], outside [n]) of the full region list -- computed once, shared, never written"""
    pl = planes(name) if colour else (gray(name),)
    out = M.patch_bytes(pl, regions(name, P), MR_SIZE, P)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- norm rows
NORM_ROW_NAMES = ("single_1p1_first", "single_2p3_last", "single_3_mid", "single_49_first", "absorb_l2", "absorb_l1", "cancel",
                  "zero", "negative_entry", "zero_sum", "random_a", "random_b")


@functools.lru_cache(None)
def norm_rows(w):
    """the planted and random rows at width w, [len(NORM_ROW_NAMES)][w] f32 (one random row less at 4096 columns)"""
    rng = np.random.RandomState(1000 + w)
    rows = []

    def single(v, at):
        r = np.zeros(w, np.float32)
        r[at] = v
        return r

    # 512 * coef * x on either side of 512 under floor: L2 1.1 -> 512, 2.3 -> 511; L1 3 -> 512, 49 -> 511
    rows += [single(1.1, 0), single(2.3, w - 1), single(3.0, w // 2), single(49.0, 0)]
    r = np.ones(w, np.float32); r[0] = 2.0 ** 27; rows.append(r)      # x0^2 = 2^54 absorbs the ones that follow in f64
    r = np.ones(w, np.float32); r[0] = 2.0 ** 53; rows.append(r)      # the same for the signed sum
    r = np.ones(w, np.float32); r[0] = 2.0 ** 53                      # ... and gives them back: in order the sum is 1
    if w >= 3:
        r[w - 2] = -2.0 ** 53
    rows.append(r)
    rows.append(np.zeros(w, np.float32))
    r = rng.uniform(0.5, 4.0, w).astype(np.float32); r[w // 3] = -0.75; rows.append(r)      # NaN at that position under RootL2
    r = np.zeros(w, np.float32)
    h = w // 2
    r[:h] = 1.0 + np.arange(h) % 7; r[h:2 * h] = -r[:h]; rows.append(r)                    # signed sum 0 (an odd width ends in 0)
    rows.append((rng.standard_normal(w) * 3.0).astype(np.float32))
    if w < 4096:
        rows.append((rng.standard_normal(w) * 50.0 + 1.0).astype(np.float32))
    out = np.stack(rows)
    out.setflags(write=False)
    return out


def take_rows(w, n):
    src = norm_rows(w)
    return src[np.arange(n) % len(src)].copy()
