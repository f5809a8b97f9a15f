"""The patches of the LIOP tests (tests/test_liop_model_cpu.py, tests/test_gpu_liop.py, tools/make_liop_fixture.py): 41 x 41 f32,
generated from integer formulas or seeded numpy, built once per process and left alone.  cases() -> list of (name, patch); meta()
-> what some cases were constructed to reach (checked against the model in tests/test_liop_model_cpu.py, never assumed).

Families:
  distinct_*        full-mantissa values, no two measurement pixels equal: the fast path, any sort by key is the reference's;
  ties_inside_*     the same with runs of equal values placed strictly inside spatial bins: ties, but no edge inside a tie group;
  edge<k>_*         one run of 40 equal values across the rank 112 k alone (k = 1 .. 5): the exact path, one edge at a time;
  edges_*           runs across several / all edges at once;
  disc_const_*      every measurement pixel equal (673 ties, the quicksort's quadratic case), the surround varies;
  two_valued_*, saturated_*   photonormalised patches that clamp: plateaus at 0 and 255, neighbour samples that tie;
  quantised_*, ramp_*   integer grey levels (the 8-bit image case): many small tie groups;
  negative_offset, subnormal   keys below zero, and keys so small that a difference of two would underflow;
  thr_lo / thr_hi   one neighbour pair whose difference sits within one f32 ulp of the threshold, below / above it: two patches
                    that differ in one pixel by one ulp (found by bisection over that pixel's bit pattern)."""
import functools

import numpy as np

import liop_model as M

L = M.L


def _base(seed):
    """smooth term + noise, full mantissas, inside (0, 255), all 1681 values distinct"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:L, 0:L].astype(np.float64)
    p = 128.0 + 60.0 * np.sin(x / (3.0 + seed % 5) + seed) * np.cos(y / (4.0 + seed % 3)) + rng.uniform(-50.0, 50.0, (L, L))
    p = p.astype(np.float32)                      # |smooth| <= 60, |noise| <= 50: inside [18, 238]
    flat = p.reshape(-1)
    while True:                                   # a repeated value moves up by one ulp until none is left
        first = np.unique(flat, return_index=True)[1]
        if len(first) == flat.size:
            return p
        dup = np.setdiff1d(np.arange(flat.size), first)
        flat[dup] = np.nextafter(flat[dup], np.float32(1e9))


def _with_runs(p, runs):
    """p with the measurement pixels of ranks [lo, hi) set to the value of rank lo, for every (lo, hi) of runs"""
    p = p.copy()
    pix = M.tables()[0]
    order = np.argsort(M.keys_of(p), kind="stable")
    flat = p.reshape(-1)
    for lo, hi in runs:
        flat[pix[order[lo:hi]]] = flat[pix[order[lo]]]
    return p


def _disc_const(value, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 255.0, (L, L)).astype(np.float32)
    p.reshape(-1)[M.tables()[0]] = np.float32(value)
    return p


def _photonorm_like(seed, gain):
    """what photometricallyNormalize leaves of a high-contrast window: 128 + gain * (x - mean), clamped to [0, 255]"""
    b = _base(seed).astype(np.float64)
    return np.clip(128.0 + gain * (b - b.mean()), 0.0, 255.0).astype(np.float32)


def _threshold_pair():
    """(thr_lo, thr_hi, (pixel i, k, t)): a sample of pixel i's neighbour k depends on a patch pixel q outside the measurement
    disc; q's value is bisected over its f32 bit patterns until nv[i][k] > nv[i][t] + threshold flips between two adjacent ones"""
    pix, sx, sy = M.tables()
    measured = set(int(v) for v in pix)
    idx, wx, wy, _, _ = M._sample_operands()
    base = _base(77)
    for i in range(M.NPIX - 1, -1, -1):
        k = 0
        ops = [int(v) for v in idx[i, k]]
        w = [(1 - wx[i, k]) * (1 - wy[i, k]), wx[i, k] * (1 - wy[i, k]), (1 - wx[i, k]) * wy[i, k], wx[i, k] * wy[i, k]]
        cand = [(w[j], ops[j]) for j in range(4) if ops[j] >= 0 and ops[j] not in measured and w[j] > 0.3]
        if not cand:
            continue
        q = max(cand)[1]
        for t in (1, 2, 3):
            if q in [int(v) for v in idx[i, t]]:
                continue

            def above(bits):
                p = base.copy()
                p.reshape(-1).view(np.uint32)[q] = bits
                nv = M.neighbour_values(p)
                thr = float(M.THRESH * (M.keys_of(p).max() - M.keys_of(p).min()))
                return float(nv[i, k]) > float(nv[i, t]) + thr, p

            lo, hi = int(np.float32(0.0).view(np.uint32)), int(np.float32(255.0).view(np.uint32))
            if above(lo)[0] or not above(hi)[0]:
                continue
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if above(mid)[0]:
                    hi = mid
                else:
                    lo = mid
            return above(lo)[1], above(hi)[1], (i, k, t)
    raise AssertionError("no threshold pair found")


@functools.lru_cache(maxsize=None)
def _build():
    E = M.EDGES
    out, meta = [], {}

    def add(name, p, **kw):
        p = np.ascontiguousarray(p, np.float32).reshape(L, L)
        assert np.isfinite(p).all()
        p.setflags(write=False)
        out.append((name, p))
        if kw:
            meta[name] = kw

    for s in range(8):
        add("distinct_%d" % s, _base(100 + s))
    add("negative_offset", _base(120) - np.float32(300.0))
    add("subnormal", (_base(121).astype(np.float64) * 1e-41).astype(np.float32))      # subnormal keys: compare, do not subtract
    for s in range(8):
        add("ties_inside_%d" % s, _with_runs(_base(200 + s), [(e - 60 - s, e - 20) for e in E] + [(600, 660)]))
    for k, e in enumerate(E):
        for s in range(2):
            add("edge%d_%d" % (k + 1, s), _with_runs(_base(300 + 10 * k + s), [(e - 20, e + 20)]), edges=(e,))
    add("edges_1_3_5", _with_runs(_base(400), [(E[0] - 20, E[0] + 20), (E[2] - 30, E[2] + 10), (E[4] - 5, E[4] + 50)]),
        edges=(E[0], E[2], E[4]))
    add("edges_all", _with_runs(_base(401), [(e - 20, e + 20) for e in E]), edges=E)
    add("edges_2_3_one_run", _with_runs(_base(402), [(E[1] - 30, E[2] + 30)]), edges=(E[1], E[2]))
    add("edge_pair_only", _with_runs(_base(403), [(E[3] - 1, E[3] + 1)]), edges=(E[3],))
    for s, v in enumerate((0.0, 255.0, 128.0, -0.0)):
        add("disc_const_%d" % s, _disc_const(v, 500 + s), disc_const=True)
    zmix = _disc_const(0.0, 510).copy()
    zmix.reshape(-1)[M.tables()[0][::2]] = np.float32(-0.0)        # -0 ties with +0
    add("disc_const_signed_zero", zmix, disc_const=True)
    y, x = np.mgrid[0:L, 0:L]
    add("two_valued_halves", np.where(x < 20, 0.0, 255.0))
    add("two_valued_diagonal", np.where(x + 2 * y < 61, 0.0, 255.0))
    add("two_valued_checker", np.where(((x // 5) + (y // 7)) % 2 == 0, 0.0, 255.0))
    add("two_valued_low_contrast", np.where((x * 7 + y * 3) % 11 < 5, 100.0, 101.0))
    for s, g in enumerate((3.0, 8.0, 40.0)):
        add("saturated_%d" % s, _photonorm_like(600 + s, g))
    half = _base(610).copy()
    half[:, 21:] = np.float32(255.0)
    add("saturated_half", half)
    for s in range(4):
        add("quantised_%d" % s, np.floor(_base(700 + s)))
    add("quantised_coarse", np.floor(_base(710) / 16.0) * 16.0)
    add("ramp_x", x.astype(np.float32) * 6.0)
    add("ramp_xy", (3 * x + 5 * y).astype(np.float32))
    lo, hi, where = _threshold_pair()
    add("thr_lo", lo, threshold_pair=where)
    add("thr_hi", hi, threshold_pair=where)
    return tuple(out), meta


def cases():
    return list(_build()[0])


def meta():
    return dict(_build()[1])


def patches():
    """[n][41][41] f32, in the order of cases()"""
    return np.stack([p for _, p in cases()])


_MODEL = []


def model():
    """[liop_model.process(patch) for every case], computed once per process"""
    if not _MODEL:
        _MODEL.extend(M.process(p) for _, p in cases())
    return list(_MODEL)
