"""Inputs of the L1 FGINN matcher's tests (vector_dist = L1: kernels_fginn32.hip with MODSX_DIST_L1, kernels_fginn_l1.hip on byte
rows), generated from seeds.  The yardstick is tests/fginn_l1_model.py; tests/test_fginn_l1_model_cpu.py proves on the CPU that the
model is the oracle's up to the chain and that these inputs reach what they claim, tests/test_gpu_fginn_l1.py runs them on the device.

Cases are the dicts of tests/fginn32_cases.py.  L1 distances are planted directly: one coordinate offset v gives the distance |v|.
The walk still compares d_0 / d_j with ratio^2 (0.64 at ratio 0.8), so the planted numbers of fginn32_cases.walk_case serve as they
are, as distances instead of squared distances."""
import numpy as np

import fginn32_cases as FC
from fginn32_cases import _Builder, EXPECT_ENDS, EXPECT_STAGE_NN50, integer_case, random_case, same_tents, unit_case, walk   # noqa: F401


class _L1Builder(_Builder):
    """_Builder with the query of cluster s at peak * e_s.  integer: offsets are rounded and spread over the following coordinates
    in parts of at most 255, so that every value stays one of the integers 0..255 (peak = 255)."""

    def __init__(self, dim, seed, peak=1000.0, integer=False):
        _Builder.__init__(self, dim, seed)
        self.peak, self.integer = peak, integer

    def cluster(self, name, dists, positions, home=(500.0, 500.0)):
        """dists: per train its L1 distance to the query, or (distance, distance in a second group of four)"""
        s = len(self.q)
        assert s + 8 < self.dim
        c = np.zeros(self.dim, np.float32)
        c[s] = self.peak
        self.q.append(c.copy())
        self.expect[s] = name
        for d, p in zip(dists, positions):
            row = c.copy()
            d, far_group = d if isinstance(d, tuple) else (d, 0.0)
            if self.integer:
                rest, k = int(round(d)), 1
                while rest > 0:
                    assert k <= 4
                    row[(s + k) % self.dim] += min(rest, 255)
                    rest, k = rest - min(rest, 255), k + 1
            else:
                row[(s + 1) % self.dim] += np.float32(d)
                row[(s + 5) % self.dim] += np.float32(far_group)      # s + 1 and s + 5 never share a group of four
            self.t.append(row)
            self.pos.append(home if p == "near" else (home[0] + 300.0, home[1]) if p == "far" else p)
        return s


def walk_case(dim=128, seed=3, integer=False):
    """fginn32_cases.walk_case with its numbers as L1 distances (times 100 and as integer rows with integer = True): one query per
    way a walk can go at ratio 0.8 and contradDist 30; `expect` names are those of EXPECT_ENDS / EXPECT_STAGE_NN50"""
    u = 100.0 if integer else 1.0
    b = _L1Builder(dim, seed, 255.0, True) if integer else _L1Builder(dim, seed)

    def at(*d):
        return [u * float(x) for x in d]

    b.cluster("record_j1", at(1, 4), ["near"] * 2)
    b.cluster("record_j3", at(1, 1.2, 1.3, 4), ["near"] * 4)
    b.cluster("record_j6", at(1, 1.1, 1.2, 1.3, 1.35, 1.4, 9), ["near"] * 7)
    b.cluster("contradiction_j1", at(1, 1.1, 4), ["near", "far", "near"])
    b.cluster("contradiction_j5", at(1, 1.1, 1.2, 1.3, 1.35, 1.4, 9), ["near"] * 5 + ["far", "near"])
    b.cluster("rank_reaches_nn", at(*np.linspace(1.0, 1.5, 60)) + at(9), ["near"] * 61)
    b.cluster("record_j48", at(*np.linspace(1.0, 1.5, 48)) + at(9), ["near"] * 49)
    b.cluster("count_above_nn", at(*np.linspace(1.0, 1.5, 50)) + at(9), ["near"] * 51)
    b.cluster("contradiction_before_many", at(1, 1.1, 1.2, 1.3, 1.31) + at(*np.linspace(1.32, 1.5, 60)), ["near"] * 4 + ["far"] + ["near"] * 60)
    b.cluster("dup_zero_near", at(0, 0, 1.0, 1.1), ["near"] * 4)
    b.cluster("dup_zero_far", at(0, 0, 1.0), ["near", "far", "near"])
    b.cluster("zero_then_positive", at(0, 1.0, 1.1), ["near"] * 3)
    return b.case()


def threshold_case(dim=128, seed=8):
    """ratio = 0.5, ratio^2 = 0.25 exactly.  d_0 / d_1 is exactly 0.25 (1 / 4: passes, <=), one ulp of the divisor below it
    (1 / (4 + ulp): passes) and one ulp of the dividend above it ((1 + ulp) / 4: fails, then the next train passes).  The dividend's
    ulp, 2^-23, comes from a second group of four."""
    b = _L1Builder(dim, seed)
    b.cluster("exact", [1.0, 4.0], ["near"] * 2)
    b.cluster("divisor_up", [1.0, float(np.nextafter(np.float32(4), np.float32(5)))], ["near"] * 2)
    b.cluster("dividend_up", [(1.0, 2.0 ** -23), 4.0, 16.0], ["near"] * 3)
    return b.case(ratio=0.5)


def subnormal_case(n1=65, n2=150, dim=36, seed=5):
    """rows around 1e-40: the INPUTS and their differences are f32 subnormals (< 1.18e-38), and so is every distance -- flushed to
    zero anywhere, every distance would be 0 and the train index alone would decide"""
    rs = np.random.RandomState(seed)
    t = (rs.randn(n2, dim) * 1e-40).astype(np.float32)
    q = (t.astype(np.float64)[rs.randint(0, n2, n1)] + 0.3e-40 * rs.randn(n1, dim)).astype(np.float32)
    q = np.where(rs.rand(n1, 1) < 0.6, q, (rs.randn(n1, dim) * 1e-40).astype(np.float32))
    return dict(q=q, t=t, pos=rs.uniform(0, 100, (n2, 2)), ratio=FC.RATIO, cd=FC.CD)


def saturating_case(n1=130, n2=300, seed=12):
    """integer rows at 128 columns over the whole range 0..255, with rows of all 0 and of all 255 on both sides: differences of 255
    in every column, the largest sum (32640) included.  Query 0 is all 255, query 1 all 0; trains 0 and 1 are all 0, train 2 all 255."""
    rs = np.random.RandomState(seed)
    t = rs.randint(0, 256, (n2, 128))
    q = np.clip(t[rs.randint(0, n2, n1)] + rs.randint(-20, 21, (n1, 128)), 0, 255)
    q = np.where(rs.rand(n1, 1) < 0.6, q, rs.randint(0, 256, (n1, 128)))
    t[0] = t[1] = 0
    t[2] = 255
    q[0], q[1] = 255, 0
    q[2:6] = np.where(rs.rand(4, 128) < 0.5, 0, 255)                    # every difference to trains 0..2 is 0 or 255
    return dict(q=q.astype(np.float32), t=t.astype(np.float32), pos=rs.uniform(0, 100, (n2, 2)), ratio=FC.RATIO, cd=FC.CD)


TIE_TILES = FC.TIE_TILES


def tie_case(geo, n1=70, dim=128, seed=9, integer=False):
    """fginn32_cases.tie_case under L1 for the geometry `geo` (mods_amd.fginn32_geometry or fginn_l1_geometry at n2 =
    tie_n2(geo)): equal distances on both sides of a tile edge, of a split edge, and at the first and last train.  integer: rows
    of integers 0..255 (dim 128)."""
    T, n2 = geo["tile"], FC.tie_n2(geo)
    edge = geo["tiles_per_split"] * T if geo["splits"] > 1 else (geo["tiles"] - 1) * T
    if edge == T:
        edge = 3 * T
    c = integer_case(n1, n2, seed) if integer else random_case(n1, n2, dim, seed, noise=0.05)
    pairs = [(T - 1, T), (edge - 1, edge), (0, n2 - 1)]
    for qi, (a, b) in enumerate(pairs):
        assert 0 <= a < b < n2
        src = 2 * T + 1 + qi
        row = c["t"][src].copy()
        c["t"][src] += 50.0
        c["t"][a], c["t"][b] = row, row
        c["pos"][a] = c["pos"][b] = (10.0 * qi, 5.0)
        c["q"][qi] = row + np.float32(1.0 if integer else 0.01)
    c["pairs"] = pairs
    return c


# ---- other summation orders (the CPU test shows that they give other results) ---------------------------------------------
def knn_f64_rounded_once(q, t, nn):
    d = np.abs(q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :]).sum(2).astype(np.float32)
    return FC._sorted_knn(d, nn)


def knn_f32_left_to_right(q, t, nn):
    d = np.zeros((len(q), len(t)), np.float32)
    e = np.abs(q[:, None, :] - t[None, :, :])                  # f32
    for k in range(q.shape[1]):
        d = d + e[:, :, k]                                     # one running f32 sum
    return FC._sorted_knn(d, nn)
