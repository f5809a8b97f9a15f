"""Inputs of the f32 FGINN matcher's tests (MatchFlannFGINN on float rows of any width: kernels_fginn32.hip, engine_fginn32.hip),
generated from seeds, plus a Python restatement of the reference's walk over a sorted neighbour list.  The yardstick of every
comparison is oracle.pyoracle (knn_linear / match_fginn); tests/test_fginn32_cases_cpu.py proves on the CPU that these inputs reach
what they claim, tests/test_gpu_fginn32.py runs them on the device.

A "case" is a dict: q [n1][dim] f32, t [n2][dim] f32, pos [n2][2] f64, ratio, cd (contradDist) and, for planted ones, `expect`:
{query index: name of what the walk of that query reaches}."""
import numpy as np

RATIO, CD = 0.8, 30.0
TENT_INT = ("q", "t0", "tj", "t1")
TENT_F64 = ("d1", "d2", "d2by2ndcl", "ratio")


def same_tents(got, ref):
    """count, indices and the f64 fields as bit patterns (NaN-safe, -0 / +0 apart)"""
    assert len(got) == len(ref), (len(got), len(ref))
    for f in TENT_INT:
        assert np.array_equal(got[f], ref[f]), f
    for f in TENT_F64:
        a, b = np.ascontiguousarray(got[f]).view(np.uint64), np.ascontiguousarray(ref[f]).view(np.uint64)
        assert np.array_equal(a, b), (f, int((a != b).sum()))


def random_case(n1, n2, dim, seed, noise=0.3):
    """Gaussian trains; six queries in ten are a train plus noise and end in a record, the others are unrelated rows: every ratio is
    near 1 and the walk goes on for as long as the neighbours lie within contradDist (three in ten do, in a 100 x 100 image)"""
    rs = np.random.RandomState(seed)
    t = rs.randn(n2, dim).astype(np.float32)
    q = (t[rs.randint(0, n2, n1)] + noise * rs.randn(n1, dim)).astype(np.float32)
    q = np.where(rs.rand(n1, 1) < 0.6, q, rs.randn(n1, dim).astype(np.float32))
    return dict(q=q, t=t, pos=rs.uniform(0, 100, (n2, 2)), ratio=RATIO, cd=CD)


def unit_case(n1, n2, dim, seed):
    """unit-norm Gaussian rows (learned descriptors); six queries in ten are a train plus noise, the others unrelated"""
    rs = np.random.RandomState(seed)
    t = rs.randn(n2, dim)
    q = t[rs.randint(0, n2, n1)] + 0.25 * rs.randn(n1, dim)
    q = np.where(rs.rand(n1, 1) < 0.6, q, rs.randn(n1, dim))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(q=q.astype(np.float32), t=t.astype(np.float32), pos=rs.uniform(0, 100, (n2, 2)), ratio=RATIO, cd=CD)


def integer_case(n1, n2, seed):
    """rows holding the integers 0..255 at dim = 128: what modsx_match_fginn takes too"""
    rs = np.random.RandomState(seed)
    t = rs.randint(0, 120, (n2, 128))
    q = np.clip(t[rs.randint(0, n2, n1)] + rs.randint(-12, 13, (n1, 128)), 0, 255)
    q = np.where(rs.rand(n1, 1) < 0.6, q, rs.randint(0, 120, (n1, 128)))
    return dict(q=q.astype(np.float32), t=t.astype(np.float32), pos=rs.uniform(0, 100, (n2, 2)), ratio=RATIO, cd=CD)


def subnormal_case(n1=65, n2=150, dim=36, seed=5):
    """entries around 1e-20: every square is an f32 subnormal (< 1.18e-38), the distances are sums of subnormals and their order
    depends on them -- flushed to zero, every distance would be 0 and the train index alone would decide"""
    rs = np.random.RandomState(seed)
    t = (rs.randn(n2, dim) * 1e-20).astype(np.float32)
    q = (t[rs.randint(0, n2, n1)] + 0.3e-20 * rs.randn(n1, dim)).astype(np.float32)
    q = np.where(rs.rand(n1, 1) < 0.6, q, (rs.randn(n1, dim) * 1e-20).astype(np.float32))
    return dict(q=q, t=t, pos=rs.uniform(0, 100, (n2, 2)), ratio=RATIO, cd=CD)


# ---- the walk, restated -------------------------------------------------------------------------------------------------
def walk(idx, dist, pos, ratio, cd, nn):
    """matching.cpp:385-457 (ratio^2 < 1) on a neighbour list sorted by (distance, index): idx / dist [n1][>= nn] (idx < 0 = no
    train).  Returns (tentatives as a list of tuples q, t0, tj, t1, d1, d2, d2by2ndcl, ratio; ends) with ends[q] = (what, j):
    what in "record", "contradiction", "nn" (rank nn reached), "trains" (the trains ran out)."""
    rsq, cd2 = ratio * ratio, cd * cd
    out, ends = [], []
    for q in range(len(idx)):
        ir, dr = idx[q], dist[q]
        end = ("nn", nn - 1)
        for j in range(1, nn):
            if j >= len(ir) or ir[j] < 0:
                end = ("trains", j)
                break
            with np.errstate(divide="ignore", invalid="ignore"):
                r = float(np.float32(dr[0]) / np.float32(dr[j]))       # f32 division, widened
            if r <= rsq:
                out.append((q, int(ir[0]), int(ir[j]), int(ir[1]), float(dr[0]), float(dr[j]), float(dr[1]), float(np.sqrt(r))))
                end = ("record", j)
                break
            dx, dy = pos[ir[0]][0] - pos[ir[j]][0], pos[ir[0]][1] - pos[ir[j]][1]
            if dx * dx + dy * dy > cd2:
                end = ("contradiction", j)
                break
        ends.append(end)
    return out, ends


def tents_array(rows, dtype):
    a = np.zeros(len(rows), dtype)
    for i, r in enumerate(rows):
        a[i] = r
    return a


def expected_stage(idx_all, dist_all, pos, ratio, cd, nn):
    """How the library closes every query (Context.debug_match_fginn_f32 `stage`), from the FULL sorted neighbour list
    (idx_all / dist_all [n1][n2]): 0 = the walk ends within j <= 3 (or nn <= 4), 1 = the resolve sweep, 2 = the resolve sweep's
    count: the first train behind j = 3 that ends the walk passes the ratio test, but its rank exceeds nn - 1."""
    rsq, cd2 = ratio * ratio, cd * cd
    _, ends = walk(idx_all, dist_all, pos, ratio, cd, min(nn, 4))
    stage = np.zeros(len(idx_all), np.uint8)
    for q, (what, j) in enumerate(ends):
        if what != "nn" or nn <= 4:
            continue
        stage[q] = 1
        ir, dr = idx_all[q], dist_all[q]
        for j in range(4, len(ir)):
            with np.errstate(divide="ignore", invalid="ignore"):
                passes = float(np.float32(dr[0]) / np.float32(dr[j])) <= rsq
            dx, dy = pos[ir[0]][0] - pos[ir[j]][0], pos[ir[0]][1] - pos[ir[j]][1]
            if passes or dx * dx + dy * dy > cd2:
                if passes and j > nn - 1:
                    stage[q] = 2
                break
    return stage


# ---- planted walks ------------------------------------------------------------------------------------------------------
class _Builder(object):
    """Every planted query sits alone at 1000 * e_s (one coordinate per query); its trains are that point plus offsets, so the
    distances inside a cluster are small, chosen numbers and every train of another cluster is ~2e6 away: it passes every ratio
    test and lies anywhere in the image."""

    def __init__(self, dim, seed):
        self.dim, self.rs = dim, np.random.RandomState(seed)
        self.q, self.t, self.pos, self.expect = [], [], [], {}

    def cluster(self, name, offsets, positions, home=(500.0, 500.0)):
        """offsets: per train a list of (coordinate shift relative to the cluster's own axis, value); positions: "near" (at home),
        "far" (more than contradDist away) or an (x, y)"""
        s = len(self.q)
        assert s + 8 < self.dim
        c = np.zeros(self.dim, np.float32)
        c[s] = 1000.0
        self.q.append(c.copy())
        self.expect[s] = name
        for off, p in zip(offsets, positions):
            row = c.copy()
            for k, v in off:
                row[(s + k) % self.dim] += np.float32(v)
            self.t.append(row)
            self.pos.append(home if p == "near" else (home[0] + 300.0, home[1]) if p == "far" else p)
        return s

    def case(self, ratio=RATIO, cd=CD):
        order = self.rs.permutation(len(self.t))            # the clusters' trains interleave over the train axis
        return dict(q=np.array(self.q, np.float32), t=np.array(self.t, np.float32)[order],
                    pos=np.array(self.pos, np.float64)[order], ratio=ratio, cd=cd, expect=dict(self.expect))


def _at(*dists):
    """trains at the given squared distances along the cluster's next axis (distance = value^2 up to rounding)"""
    return [[(1, float(np.sqrt(d)))] for d in dists]


def walk_case(dim=128, seed=3):
    """One query per way a walk can go, at ratio 0.8 (ratio^2 = 0.64) and contradDist 30.  `expect` names are checked on the CPU for
    nn = 2, 4 and 50 (EXPECT_ENDS)."""
    b = _Builder(dim, seed)
    b.cluster("record_j1", _at(1, 4), ["near"] * 2)
    b.cluster("record_j3", _at(1, 1.2, 1.3, 4), ["near"] * 4)
    b.cluster("record_j6", _at(1, 1.1, 1.2, 1.3, 1.35, 1.4, 9), ["near"] * 7)
    b.cluster("contradiction_j1", _at(1, 1.1, 4), ["near", "far", "near"])
    b.cluster("contradiction_j5", _at(1, 1.1, 1.2, 1.3, 1.35, 1.4, 9), ["near"] * 5 + ["far", "near"])
    b.cluster("rank_reaches_nn", _at(*np.linspace(1.0, 1.5, 60)) + _at(9), ["near"] * 61)
    # 47 trains fail the ratio test nearby, the 48th passes: rank 48 <= nn - 1 = 49 is reached, a record at j = 48 ...
    b.cluster("record_j48", _at(*np.linspace(1.0, 1.5, 48)) + _at(9), ["near"] * 49)
    # ... and with one more it is rank 50: the count bounds the rank above nn - 1, no record
    b.cluster("count_above_nn", _at(*np.linspace(1.0, 1.5, 50)) + _at(9), ["near"] * 51)
    # a contradictive train at rank 4 in front of 60 that do not end the walk: the bound 3 + 60 + 1 says nothing, the train ends it
    b.cluster("contradiction_before_many", _at(1, 1.1, 1.2, 1.3, 1.31) + _at(*np.linspace(1.32, 1.5, 60)), ["near"] * 4 + ["far"] + ["near"] * 60)
    b.cluster("dup_zero_near", [[], []] + _at(1.0, 1.1), ["near"] * 4)           # d0 = d1 = 0: 0 / 0 at j = 1, then 0 / 1 passes
    b.cluster("dup_zero_far", [[], []] + _at(1.0), ["near", "far", "near"])       # 0 / 0, then the contradiction
    b.cluster("zero_then_positive", [[]] + _at(1.0, 1.1), ["near"] * 3)           # d0 = 0 < d1: ratio 0 at j = 1
    return b.case()


# what the walk of every planted query reaches, per nn: (what, j)
EXPECT_ENDS = {
    "record_j1": {2: ("record", 1), 4: ("record", 1), 50: ("record", 1)},
    "record_j3": {2: ("nn", 1), 4: ("record", 3), 50: ("record", 3)},
    "record_j6": {2: ("nn", 1), 4: ("nn", 3), 50: ("record", 6)},
    "contradiction_j1": {2: ("contradiction", 1), 4: ("contradiction", 1), 50: ("contradiction", 1)},
    "contradiction_j5": {2: ("nn", 1), 4: ("nn", 3), 50: ("contradiction", 5)},
    "rank_reaches_nn": {2: ("nn", 1), 4: ("nn", 3), 50: ("nn", 49)},
    "record_j48": {2: ("nn", 1), 4: ("nn", 3), 50: ("record", 48)},
    "count_above_nn": {2: ("nn", 1), 4: ("nn", 3), 50: ("nn", 49)},
    "contradiction_before_many": {2: ("nn", 1), 4: ("nn", 3), 50: ("contradiction", 4)},
    "dup_zero_near": {2: ("nn", 1), 4: ("record", 2), 50: ("record", 2)},
    "dup_zero_far": {2: ("contradiction", 1), 4: ("contradiction", 1), 50: ("contradiction", 1)},
    "zero_then_positive": {2: ("record", 1), 4: ("record", 1), 50: ("record", 1)},
}
# the library's stage per planted query at nn = 50 (0 host walk, 1 resolve sweep, 2 its count); at nn = 2 and 4 every stage is 0
EXPECT_STAGE_NN50 = {"record_j1": 0, "record_j3": 0, "record_j6": 1, "contradiction_j1": 0, "contradiction_j5": 1,
                     "rank_reaches_nn": 2, "record_j48": 1, "count_above_nn": 2, "contradiction_before_many": 1,
                     "dup_zero_near": 0, "dup_zero_far": 0, "zero_then_positive": 0}


def short_case(dim=128, seed=4):
    """n2 = 6 < nn = 50: no train passes the ratio test, all are near -- at nn = 50 the walk runs out of trains behind the fourth
    neighbour (the resolve sweep finds nothing that ends it)"""
    b = _Builder(dim, seed)
    b.cluster("out_of_trains", _at(1, 1.1, 1.2, 1.25, 1.3, 1.35), ["near"] * 6)
    c = b.case()
    c["expect_ends"] = {2: ("nn", 1), 4: ("nn", 3), 50: ("trains", 6)}
    return c


def tiny_case(dim=128, seed=6):
    """n2 = 3 < 4: the fourth key does not exist"""
    b = _Builder(dim, seed)
    b.cluster("three_trains", _at(1, 1.1, 1.2), ["near"] * 3)
    c = b.case()
    c["expect_ends"] = {2: ("nn", 1), 4: ("trains", 3), 50: ("trains", 3)}
    return c


def threshold_case(dim=128, seed=8):
    """ratio = 0.5, ratio^2 = 0.25 exactly.  d_0 / d_1 is exactly 0.25 (1 / 4: passes, <=), one ulp of the divisor below it
    (1 / (4 + ulp): passes) and one ulp of the dividend above it ((1 + ulp) / 4: fails, then the next train passes).  The ulps come
    from a second group of four: 4 + 0.0007^2 rounds to the f32 behind 4, 1 + 0.00035^2 to the f32 behind 1."""
    b = _Builder(dim, seed)
    b.cluster("exact", [[(1, 1.0)], [(1, 2.0)]], ["near"] * 2)
    b.cluster("divisor_up", [[(1, 1.0)], [(1, 2.0), (5, 0.0007)]], ["near"] * 2)
    b.cluster("dividend_up", [[(1, 1.0), (5, 0.00035)], [(1, 2.0)], [(1, 3.0)]], ["near"] * 3)
    return b.case(ratio=0.5)


# ---- planted ties -------------------------------------------------------------------------------------------------------
def tie_case(geo, n1=70, dim=128, seed=9):
    """Equal f32 distances on both sides of a tile edge and of a split edge of the geometry `geo` (mods_amd.fginn32_geometry for
    n2 = tie_n2(geo)): query 0's two nearest trains are copies of one row at the last index of tile 0 and the first of tile 1, query
    1's stand at the last index of split 0 and the first of split 1 (with one split: around the last tile edge), query 2's at index 0
    and the last index.  The copies share one position, so j = 1 (ratio 1) fails without contradiction and j = 2, a far row, gives the
    record: t0 and t1 are the two copies, lower index first."""
    T, n2 = geo["tile"], tie_n2(geo)
    edge = geo["tiles_per_split"] * T if geo["splits"] > 1 else (geo["tiles"] - 1) * T
    if edge == T:                                            # one tile per split: query 0 has that edge, query 1 takes another one
        edge = 3 * T
    c = random_case(n1, n2, dim, seed, noise=0.05)
    pairs = [(T - 1, T), (edge - 1, edge), (0, n2 - 1)]
    for qi, (a, b) in enumerate(pairs):
        assert 0 <= a < b < n2
        src = 2 * T + 1 + qi                                 # a row of tile 2, no edge near it
        row = c["t"][src].copy()
        c["t"][src] += 50.0                                  # the original moves away; its two copies stay
        c["t"][a], c["t"][b] = row, row
        c["pos"][a] = c["pos"][b] = (10.0 * qi, 5.0)
        c["q"][qi] = row + np.float32(0.01)
    c["pairs"] = pairs
    return c


def tie_n2(geo):
    return geo["tiles"] * geo["tile"] - 2


TIE_TILES = 6      # the tie case has this many tiles, whatever the split count


# ---- other summation orders (the CPU test shows that they give other results) ---------------------------------------------
def knn_f64_rounded_once(q, t, nn):
    d = ((q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :]) ** 2).sum(2).astype(np.float32)
    return _sorted_knn(d, nn)


def knn_f32_left_to_right(q, t, nn):
    d = np.zeros((len(q), len(t)), np.float32)
    e = q[:, None, :] - t[None, :, :]                          # f32
    for k in range(q.shape[1]):
        d = d + e[:, :, k] * e[:, :, k]                        # f32 products, one running f32 sum
    return _sorted_knn(d, nn)


def _sorted_knn(d, nn):
    n1, n2 = d.shape
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n2, dtype=np.uint64)[None, :]
    order = np.argsort(key, axis=1)[:, :nn]
    idx = np.full((n1, nn), -1, np.int32)
    dist = np.full((n1, nn), np.finfo(np.float32).max, np.float32)
    idx[:, :order.shape[1]] = order
    dist[:, :order.shape[1]] = np.take_along_axis(d, order, 1)
    return idx, dist
