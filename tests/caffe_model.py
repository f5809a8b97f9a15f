"""A numpy restatement of what the reference's "CAFFE" branch (imagerepresentation.cpp:1343-1534) does around its network: the
arguments it calls interpolate with, the bytes of convertTo(CV_8UC3) / CV_8U + GRAY2BGR, the blob of CVMatToDatum minus the
truncated mean, and L2normalize / L1normalize / RootNormalize (:181-217).  The samples themselves are the oracle's interpolate
(oracle.pyoracle.interpolate), which tests/test_caffe_model_cpu.py ties to the compiled reference; the norms are tied to what the
reference's three functions computed (tests/golden/caffe_norm_ref.npz)."""
import numpy as np

from oracle import pyoracle as O

NORM_L2, NORM_L1, NORM_ROOTL2, NORM_NONE = 0, 1, 2, 3
KP = ("x", "y", "a11", "a12", "a21", "a22")


def jobs(regs, mr_size, P):
    """dict(curr_sc, x, y, a11, a12, a21, a22: [n] f32) -- :1368-1370, :1395, :1400-1406"""
    patch_image_size = 2 * int(mr_size) + 1
    image_to_patch_scale = float(patch_image_size) / float(P)
    k = regs["reproj_kp"]
    sc = (image_to_patch_scale * k["s"].astype(np.float64)).astype(np.float32)        # the f64 product, rounded once
    d = dict(curr_sc=sc, x=k["x"].astype(np.float32), y=k["y"].astype(np.float32))
    for f in KP[2:]:
        d[f] = k[f].astype(np.float32) * sc                                           # f32 products
    return d


def border(j, rows, cols, P):
    """interpolateCheckBorders for every job on planes of rows x cols -> bool [n]"""
    n = len(j["x"])
    if not n:
        return np.zeros(0, bool)
    t = np.stack([np.full(n, cols, np.float64), np.full(n, rows, np.float64)] + [j[f].astype(np.float64) for f in KP] +
                 [np.full(n, P, np.float64)], 1)
    return O.interpolate_check_borders(t)


def samples(planes, j, P, interpolate=None):
    """(f32 [n][len(planes)][P][P], outside [n] bool): interpolate of every plane at every job's arguments; outside = what
    interpolate returns (the same for every plane: it depends on the coordinates alone)"""
    interpolate = interpolate or O.interpolate
    n = len(j["x"])
    out = np.zeros((n, len(planes), P, P), np.float32)
    outside = np.zeros(n, bool)
    for i in range(n):
        for c, pl in enumerate(planes):
            out[i, c], t = interpolate(pl, *(j[f][i] for f in KP), P, P)
            outside[i] |= t
    return out, outside


def to_bytes(v):
    """saturate_cast<uchar>(float): round to nearest, ties to even, clamp to 0 .. 255"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def patch_bytes(planes, regs, mr_size, P):
    """(u8 [n][3][P][P], border [n] bool, outside [n] bool); a single plane is gray: its byte in all three channels"""
    rows, cols = planes[0].shape
    j = jobs(regs, mr_size, P)
    v, outside = samples(planes, j, P)
    b = to_bytes(v)
    if len(planes) == 1:
        b = np.repeat(b, 3, axis=1)
    return b, border(j, rows, cols, P), outside


def blob(b, mean):
    """[n][3][P][P] f32 = (float)byte - (float)(int)mean[c]: mean_px is a vector<int> assigned from doubles"""
    m = np.array([int(x) for x in mean], np.float32)
    return b.astype(np.float32) - m[None, :, None, None]


def flags(border_, outside):
    return (border_.astype(np.uint8) | (outside.astype(np.uint8) << 1)).astype(np.uint8)


def row_sums(rows, norm, order=None):
    """the f64 norm of every row: a Python loop over the columns in `order` (default 0 .. dim - 1, the reference's), vectorised
    over the rows"""
    x = np.ascontiguousarray(rows, np.float32)
    acc = np.zeros(len(x), np.float64)
    for i in (range(x.shape[1]) if order is None else order):
        acc += (x[:, i] * x[:, i]).astype(np.float64) if norm == NORM_L2 else x[:, i].astype(np.float64)
    return acc


def finish_rows(rows, norm, acc):
    x = np.ascontiguousarray(rows, np.float32)
    with np.errstate(all="ignore"):
        coef = 1.0 / np.sqrt(acc) if norm == NORM_L2 else 1.0 / acc
        v = (512.0 * coef)[:, None] * x.astype(np.float64)
        return (np.sqrt(v) if norm == NORM_ROOTL2 else np.floor(v)).astype(np.float32)


def norm_rows(rows, norm):
    x = np.ascontiguousarray(rows, np.float32)
    if norm == NORM_NONE or not x.size:
        return x.copy()
    return finish_rows(x, norm, row_sums(x, norm))


def pairwise_sums(rows, norm):
    """the same terms added as a balanced tree -- NOT the reference's order"""
    x = np.ascontiguousarray(rows, np.float32)
    t = (x * x).astype(np.float64) if norm == NORM_L2 else x.astype(np.float64)
    while t.shape[1] > 1:
        if t.shape[1] % 2:
            t = np.concatenate([t, np.zeros((len(t), 1))], 1)
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]
