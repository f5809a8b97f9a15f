"""CPU: the inputs of tests/test_gpu_fginn32.py are fit for what they claim (oracle only), and the library's host-side pieces of the
f32 FGINN matcher that need no device: the d_pass bisection."""
import numpy as np
import pytest

import fginn32_cases as FC


def _oracle_walk(oracle, c, nn):
    idx, dist = oracle.knn_linear(c["q"], c["t"], nn)
    rows, ends = FC.walk(idx, dist, c["pos"], c["ratio"], c["cd"], nn)
    ref = oracle.match_fginn(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], nn)
    FC.same_tents(FC.tents_array(rows, ref.dtype), ref)          # the restated walk is the oracle's
    return idx, dist, ends, ref


def test_the_summation_order_matters(oracle):
    """f64 sums rounded once, or f32 sums in plain left-to-right order, give another tentative list than the oracle's groups of
    four: a kernel with another order fails the GPU comparison"""
    c = FC.random_case(64, 200, 36, 11)
    nn = 50
    _, _, _, ref = _oracle_walk(oracle, c, nn)
    assert len(ref) > 20
    for other in (FC.knn_f64_rounded_once, FC.knn_f32_left_to_right):
        idx, dist = other(c["q"], c["t"], nn)
        rows, _ = FC.walk(idx, dist, c["pos"], c["ratio"], c["cd"], nn)
        got = FC.tents_array(rows, ref.dtype)
        differs = len(got) != len(ref) or any(
            not np.array_equal(np.ascontiguousarray(got[f]).view(np.uint64), np.ascontiguousarray(ref[f]).view(np.uint64)) for f in FC.TENT_F64)
        assert differs, other.__name__
    # and the model of the order itself: groups of four
    q, t = c["q"], c["t"]
    e = q[:, None, :] - t[None, :, :]
    p = e * e
    d = np.zeros((len(q), len(t)), np.float32)
    for k in range(0, q.shape[1], 4):
        d = d + (((p[:, :, k] + p[:, :, k + 1]) + p[:, :, k + 2]) + p[:, :, k + 3])
    idx, dist = FC._sorted_knn(d, nn)
    oi, od = oracle.knn_linear(q, t, nn)
    assert np.array_equal(idx, oi) and np.array_equal(dist.view(np.uint32), od.view(np.uint32))


@pytest.mark.parametrize("nn", [2, 4, 50])
def test_walk_case_reaches_every_end(oracle, nn):
    c = FC.walk_case()
    assert set(c["expect"].values()) == set(FC.EXPECT_ENDS) == set(FC.EXPECT_STAGE_NN50)
    _, _, ends, ref = _oracle_walk(oracle, c, nn)
    for q, name in c["expect"].items():
        assert ends[q] == FC.EXPECT_ENDS[name][nn], (name, nn, ends[q])
    n2 = len(c["t"])
    ia, da = oracle.knn_linear(c["q"], c["t"], n2)
    stage = FC.expected_stage(ia, da, c["pos"], c["ratio"], c["cd"], nn)
    for q, name in c["expect"].items():
        assert stage[q] == (FC.EXPECT_STAGE_NN50[name] if nn == 50 else 0), (name, nn)
    if nn == 50:
        assert {0, 1, 2} == set(int(x) for x in stage)
        kinds = {e[0] for e in ends}
        assert kinds == {"record", "contradiction", "nn"}
        assert any(e == ("record", j) for e in ends for j in (1,)) and any(e[0] == "record" and 2 <= e[1] <= 3 for e in ends)
        assert any(e[0] == "record" and e[1] >= 4 for e in ends)


def test_zero_distances(oracle):
    """0 / 0 on both sides of the contradiction distance, and d_0 = 0 < d_1"""
    c = FC.walk_case()
    idx, dist, ends, ref = _oracle_walk(oracle, c, 50)
    byname = {v: k for k, v in c["expect"].items()}
    for name in ("dup_zero_near", "dup_zero_far"):
        q = byname[name]
        assert dist[q, 0] == 0 and dist[q, 1] == 0 and idx[q, 0] < idx[q, 1]
    q = byname["dup_zero_near"]
    r = ref[ref["q"] == q][0]
    assert r["d1"] == 0 and r["d2"] > 0 and r["ratio"] == 0 and r["d2by2ndcl"] == 0 and r["tj"] != r["t1"]
    assert byname["dup_zero_far"] not in ref["q"]
    q = byname["zero_then_positive"]
    assert dist[q, 0] == 0 < dist[q, 1]
    r = ref[ref["q"] == q][0]
    assert r["ratio"] == 0 and r["tj"] == r["t1"]


@pytest.mark.parametrize("make", [FC.short_case, FC.tiny_case])
def test_fewer_trains_than_nn(oracle, make):
    c = make()
    assert len(c["t"]) < 50
    for nn in (2, 4, 50):
        _, _, ends, ref = _oracle_walk(oracle, c, nn)
        assert ends[0] == c["expect_ends"][nn] and len(ref) == 0


def test_threshold_case_sits_on_the_threshold(oracle):
    c = FC.threshold_case()
    rsq = c["ratio"] ** 2
    assert rsq == 0.25
    idx, dist, ends, ref = _oracle_walk(oracle, c, 50)
    byname = {v: k for k, v in c["expect"].items()}
    one, four = np.float32(1), np.float32(4)
    q = byname["exact"]
    assert dist[q, 0] == one and dist[q, 1] == four and float(dist[q, 0] / dist[q, 1]) == rsq and ends[q] == ("record", 1)
    q = byname["divisor_up"]
    assert dist[q, 0] == one and dist[q, 1] == np.nextafter(four, np.float32(5)) and float(dist[q, 0] / dist[q, 1]) < rsq
    assert ends[q] == ("record", 1)
    q = byname["dividend_up"]
    assert dist[q, 0] == np.nextafter(one, np.float32(2)) and dist[q, 1] == four and float(dist[q, 0] / dist[q, 1]) > rsq
    assert ends[q] == ("record", 2)


def test_subnormal_case_depends_on_subnormals(oracle):
    c = FC.subnormal_case()
    idx, dist, ends, ref = _oracle_walk(oracle, c, 50)
    tiny = np.finfo(np.float32).tiny
    assert (dist[:, :8] < tiny).all() and (dist[:, 1] > 0).all()            # every distance in reach is a subnormal
    assert len(ref) > 10
    assert not np.array_equal(idx[:, 0], np.zeros(len(idx), np.int32))       # flushed to zero, train 0 would win everywhere
    e = c["q"][:, None, :] - c["t"][None, :, :]
    assert ((e * e)[e != 0] < tiny).all()


@pytest.mark.parametrize("splits", [0, 1, 2, 3, 1 << 20])
def test_tie_case_straddles_tile_and_split_edges(modsx, oracle, splits):
    n1, dim = 70, 128
    T = modsx.fginn32_geometry(n1, 1000, dim)["tile"]
    geo = modsx.fginn32_geometry(n1, FC.TIE_TILES * T - 2, dim, splits)
    assert geo["tiles"] == FC.TIE_TILES and FC.tie_n2(geo) == FC.TIE_TILES * T - 2
    c = FC.tie_case(geo, n1, dim)
    idx, dist, ends, ref = _oracle_walk(oracle, c, 50)
    tps = geo["tiles_per_split"]
    for qi, (a, b) in enumerate(c["pairs"]):
        assert idx[qi, 0] == a and idx[qi, 1] == b and dist[qi, 0] == dist[qi, 1] > 0      # the lower index first
        r = ref[ref["q"] == qi][0]
        assert (r["t0"], r["t1"]) == (a, b) and r["tj"] not in (a, b) and ends[qi] == ("record", 2)
    a, b = c["pairs"][0]
    assert a // T + 1 == b // T                                                             # a tile edge
    a, b = c["pairs"][1]
    assert a // T + 1 == b // T
    if geo["splits"] > 1:
        assert (a // T) // tps + 1 == (b // T) // tps                                       # a split edge
    a, b = c["pairs"][2]
    assert a == 0 and (b // T) // tps == geo["splits"] - 1                                  # first and last split


def test_dpass_bisection_against_brute_force(modsx):
    """d_pass = the smallest f32 d > 0 with f64(f32(d0 / d)) <= ratio^2: the bit patterns around the library's answer"""
    rs = np.random.RandomState(17)
    n = 10000
    d0 = np.exp(rs.uniform(np.log(1e-44), np.log(1e36), n)).astype(np.float32)
    d0[:50] = 0
    d0[50:100] = rs.randint(0, 1000, 50)
    ratio = rs.uniform(0.0, 0.9999, n)
    ratio[100:150] = 0.5
    ratio[150:160] = 0.0
    got = modsx.fginn32_dpass(d0, ratio)
    bits = got.view(np.uint32).astype(np.int64)
    rsq = ratio * ratio

    def passes(b):
        d = np.clip(b, 0, 0x7f800000).astype(np.uint32).view(np.float32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            return (d0 / d).astype(np.float64) <= rsq

    assert (bits >= 1).all() and (bits <= 0x7f800000).all()
    assert passes(bits).all()
    for k in range(1, 9):
        below = bits - k
        assert (~passes(below) | (below < 1)).all(), k                 # nothing below it passes (0 / 0 is NaN at pattern 0)
        assert passes(bits + k).all(), k                               # everything above it does
    assert (got[:50] == np.float32(1e-45)).all()                      # d0 = 0: the smallest subnormal
    assert np.isinf(got[(ratio == 0) & (d0 > 1)]).all()               # ratio 0: only a quotient that underflows to 0 passes
