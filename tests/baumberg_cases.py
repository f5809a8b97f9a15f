"""Inputs of the Baumberg parity tests (tests/test_baumberg_cases_cpu.py, tests/test_gpu_baumberg.py): seeded planes and a job
list of about 1 300 keypoints, the oracle's answers for them, and a numpy restatement of the slot schedule of k_baumberg_stream
(mods_amd/csrc/kernels_affine.hip).  No GPU in here.

Planes (`planes(oracle)`): three blurred blob planes, 64 x 80, 33 x 47 and 24 x 24 (the last is smaller than most sampled
windows), a constant 40 x 40 plane (all gradients 0: the NaN exit at iteration 0) and a 48 x 56 ridge plane (one dominant
gradient direction: the anisotropy exit).

Keypoints (`jobs()`): per plane, positions uniform from 2 px outside one side to 2 px outside the other, s = 1.6 pd f with
f in SCALES and pixelDistance pd in PDS, x and y scaled by pd; and planted ones: windows wholly outside the plane, centres
exactly on pixel 1 and on cols - 3 / rows - 3, first-iteration window corners exactly on those values and one ulp either side,
small windows in the middle of the constant plane.  The lists of the planes are interleaved in job order, so that the two slots of
a wavefront hold planes of different sizes.
"""
import numpy as np

from mods_amd import synthetic

W = 19
SCALES = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0)
PDS = (1.0, 2.0, 4.0, 8.0)
BLOB_PLANES = ((64, 80, 60, 4101), (33, 47, 24, 4102), (24, 24, 10, 4103))   # rows, cols, blobs, seed
FLAT, RIDGE = 3, 4                                                           # plane indices
PER_BLOB_PLANE, PER_FLAT, PER_RIDGE = 275, 20, 150
KEY_SEED = 9001
REASONS = ("converged", "nan", "negative discriminant", "anisotropy", "iteration limit")
TOUCH_ALWAYS, TOUCH_NEVER, TOUCH_MIXED = 1, 2, 3

_planes = None
_oracle_cache = {}


def planes(oracle):
    """the five planes, f32, built once"""
    global _planes
    if _planes is None:
        out = [oracle.gaussian_blur(synthetic.blob_image(r, c, nb, seed), 1.6) for r, c, nb, seed in BLOB_PLANES]
        out.append(np.full((40, 40), 90.0, np.float32))
        rs = np.random.RandomState(4105)
        yy, xx = np.mgrid[0:48, 0:56].astype(np.float64)
        ridge = 128.0 + 70.0 * np.sin(0.55 * xx + 0.08 * yy) + rs.uniform(-1.5, 1.5, xx.shape)
        out.append(oracle.gaussian_blur(ridge.astype(np.float32), 1.6))
        _planes = [np.ascontiguousarray(p, np.float32) for p in out]
    return _planes


def plane_shapes():
    return [(r, c) for r, c, _, _ in BLOB_PLANES] + [(40, 40), (48, 56)]


def _uniform(rs, rows, cols, count):
    """count keypoints: position uniform from 2 px outside to 2 px outside (plane pixels), scale factor and pixelDistance drawn"""
    lx = rs.uniform(-2.0, cols + 2.0, count)
    ly = rs.uniform(-2.0, rows + 2.0, count)
    f = np.array(SCALES)[rs.randint(0, len(SCALES), count)]
    pd = np.array(PDS)[rs.randint(0, len(PDS), count)]
    return [(lx[i] * pd[i], ly[i] * pd[i], 1.6 * pd[i] * f[i], pd[i]) for i in range(count)]


def _planted(rows, cols):
    """keypoints placed on the values where the border test and the two sampling branches meet (plane pixels x pd)"""
    out = []
    one = np.float32(1.0)
    for pd in (1.0, 4.0):
        cx, cy = np.float32(cols - 3), np.float32(rows - 3)
        mx, my = 0.5 * cols, 0.5 * rows
        # centres exactly on pixel 1 and on cols - 3 / rows - 3
        for f in (0.5, 1.0):
            for lx, ly in ((one, my), (cx, my), (mx, one), (mx, cy), (one, one), (cx, cy)):
                out.append((float(lx) * pd, float(ly) * pd, 1.6 * pd * f, pd))
        # first-iteration corners exactly on 1 / cols - 3 / rows - 3 (corner = centre -+ 10 * 0.5), and one ulp either side
        for base, axis in ((np.float32(6.0), 0), (np.float32(cols - 8), 0), (np.float32(6.0), 1), (np.float32(rows - 8), 1)):
            for v in (np.nextafter(base, np.float32(-1e9)), base, np.nextafter(base, np.float32(1e9))):
                lx, ly = (float(v), my) if axis == 0 else (mx, float(v))
                out.append((lx * pd, ly * pd, 1.6 * pd * 0.5, pd))
    # windows wholly outside the plane, on all four sides
    for lx, ly in ((-45.0, 0.5 * rows), (cols + 45.0, 0.5 * rows), (0.5 * cols, -45.0), (0.5 * cols, rows + 45.0)):
        out.append((lx * 2.0, ly * 2.0, 1.6 * 2.0, 2.0))
    return out


_jobs = None


def jobs():
    """-> (plane_of int32 [n], xyspd f32 [n, 4]): the whole case list, planes interleaved in job order"""
    global _jobs
    if _jobs is None:
        rs = np.random.RandomState(KEY_SEED)
        shapes = plane_shapes()
        lists = []
        for pi, (r, c) in enumerate(shapes):
            if pi == FLAT:
                lst = _uniform(rs, r, c, PER_FLAT)
                # small windows in the middle of the constant plane: every sample inside, every gradient 0
                lx, ly = rs.uniform(13.0, 26.0, 40), rs.uniform(13.0, 26.0, 40)
                f = np.array(SCALES[:3])[rs.randint(0, 3, 40)]
                pd = np.array(PDS)[rs.randint(0, len(PDS), 40)]
                lst += [(lx[i] * pd[i], ly[i] * pd[i], 1.6 * pd[i] * f[i], pd[i]) for i in range(40)]
            else:
                lst = _uniform(rs, r, c, PER_RIDGE if pi == RIDGE else PER_BLOB_PLANE)
            planted = _planted(r, c)
            # planted keypoints spread through the plane's list
            step = max(1, len(lst) // len(planted))
            for i, k in enumerate(planted):
                lst.insert(min(len(lst), i * (step + 1)), k)
            lists.append(lst)
        plane_of, rows = [], []
        for i in range(max(len(l) for l in lists)):
            for pi, l in enumerate(lists):
                if i < len(l):
                    plane_of.append(pi)
                    rows.append(l[i])
        _jobs = (np.array(plane_of, np.int32), np.array(rows, np.float32).reshape(-1, 4))
        assert np.isfinite(_jobs[1]).all() and (_jobs[1][:, 3] > 0).all()
    return _jobs


def subset(count, start=0):
    """a slice of the case list (it keeps the interleaving)"""
    po, xy = jobs()
    return po[start:start + count], xy[start:start + count]


def oracle_results(oracle, plane_of=None, xyspd=None, **params):
    """oracle.find_affine_shape_batch for (a slice of) the case list under the given parameters, cached per (jobs, parameters)"""
    if plane_of is None:
        plane_of, xyspd = jobs()
    key = (plane_of.tobytes(), xyspd.tobytes(), tuple(sorted(params.items())))
    if key not in _oracle_cache:
        res = oracle.find_affine_shape_batch(planes(oracle), plane_of, xyspd, oracle.default_params(**params))
        for v in res.values():
            v.setflags(write=False)
        _oracle_cache[key] = res
    return _oracle_cache[key]


def passes_of(res, max_iterations=16):
    """iterations the stream kernel runs for every keypoint: the loop counter at a break + 1, maxIterations when the loop ran out"""
    return np.where(res["reason"] == 4, max_iterations, res["iters"] + 1).astype(np.int64)


# ---- the slot schedule of k_baumberg_stream<K> ------------------------------------------------------------------------------------

def xcd_chunk(b, nchunks):
    """kmath.hpp xcd_chunk: the chunk workgroup b takes (>= nchunks: none)"""
    per = (nchunks + 7) >> 3
    return (b & 7) * per + (b >> 3)


def schedule(passes, chunk, K=2):
    """Which slot ran which keypoint in which pass.  passes[k] = iterations keypoint k runs (>= 1).  One entry per wavefront with
    work (chunk index c = keypoints c * chunk ..): a list of passes, each a tuple of K job indices (-1 = the slot is idle) and a
    tuple of the slots filled at the head of that pass.  Refill in slot order; a slot is free again in the pass after its
    keypoint's last iteration."""
    n = len(passes)
    nchunks = (n + chunk - 1) // chunk
    waves = []
    for c in range(nchunks):
        nxt, end = c * chunk, min(c * chunk + chunk, n)
        job, left, rows = [-1] * K, [0] * K, []
        while True:
            filled = []
            idle = [q for q in range(K) if job[q] < 0]
            for rank, q in enumerate(idle):
                if nxt + rank < end:
                    job[q], left[q] = nxt + rank, int(passes[nxt + rank])
                    filled.append(q)
            nxt = min(nxt + len(idle), end)
            if all(j < 0 for j in job):
                break
            rows.append((tuple(job), tuple(filled)))
            for q in range(K):
                if job[q] >= 0:
                    left[q] -= 1
                    if left[q] == 0:
                        job[q] = -1
        waves.append(rows)
    return waves


def schedule_patterns(wave):
    """the refill patterns one wavefront of schedule() shows (K = 2)"""
    out = set()
    one_idle = 0
    for p, (job, filled) in enumerate(wave):
        if p > 0 and filled == (0,) and job[1] >= 0:
            out.add("refill slot 0 while slot 1 is live")
        if p > 0 and filled == (1,) and job[0] >= 0:
            out.add("refill slot 1 while slot 0 is live")
        if p > 0 and filled == (0, 1):
            out.add("refill both slots in the same pass")
        one_idle += (job[0] < 0) != (job[1] < 0)
    if one_idle >= 3:
        out.add("three passes with one slot idle")
    last = wave[-1][0]
    if last[0] >= 0 and last[1] < 0:
        out.add("chunk ends in slot 0")
    if last[1] >= 0 and last[0] < 0:
        out.add("chunk ends in slot 1")
    return out


PATTERNS = ("refill slot 0 while slot 1 is live", "refill slot 1 while slot 0 is live", "refill both slots in the same pass",
            "three passes with one slot idle", "chunk ends in slot 0", "chunk ends in slot 1")
