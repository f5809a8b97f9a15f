"""CPU: the numpy model of the L1 FGINN search (tests/fginn_l1_model.py) is the oracle's in everything but the chain, its L1 chain
is the restated FLANN functor, and the inputs of tests/test_gpu_fginn_l1.py (tests/fginn_l1_cases.py) reach what they claim."""
import numpy as np
import pytest

import fginn32_cases as FC
import fginn_l1_cases as LC
import fginn_l1_model as LM


def _cases():
    yield "random36", FC.random_case(64, 200, 36, 11)
    yield "random128", FC.random_case(65, 130, 128, 12)
    yield "unit256", FC.unit_case(33, 90, 256, 13)
    yield "integer", FC.integer_case(60, 140, 13)
    yield "walk_l2", FC.walk_case()
    yield "walk_l1", LC.walk_case()
    yield "walk_l1_int", LC.walk_case(integer=True)
    yield "threshold_l2", FC.threshold_case()
    yield "threshold_l1", LC.threshold_case()
    yield "subnormal_l2", FC.subnormal_case()
    yield "subnormal_l1", LC.subnormal_case()
    yield "saturating", LC.saturating_case()
    yield "short", FC.short_case()
    yield "tiny", FC.tiny_case()


def _differs(got, ref):
    return len(got) != len(ref) or any(
        not np.array_equal(np.ascontiguousarray(got[f]).view(np.uint64), np.ascontiguousarray(ref[f]).view(np.uint64))
        for f in FC.TENT_F64) or any(not np.array_equal(got[f], ref[f]) for f in FC.TENT_INT)


@pytest.mark.parametrize("nn", [2, 4, 50])
def test_the_model_with_the_l2_chain_is_the_oracle(modsx, oracle, nn):
    """sort, key, tie rule and walk are pinned: only the chain's one line is the model's own"""
    for name, c in _cases():
        ref = oracle.match_fginn(c["q"], c["t"], c["pos"], c["ratio"], c["cd"], nn)
        FC.same_tents(LM.match(c, nn, "l2"), ref)
        idx, dist = LM.knn(c["q"], c["t"], nn, "l2")
        oi, od = oracle.knn_linear(c["q"], c["t"], nn)
        assert np.array_equal(idx, oi), name
        assert np.array_equal(dist.view(np.uint32)[idx >= 0], od.view(np.uint32)[oi >= 0]), name


def test_the_l1_chain_on_integer_rows_is_the_integer_sum(modsx):
    for c in (FC.integer_case(60, 140, 13), LC.saturating_case(), LC.walk_case(integer=True)):
        for nn in (4, 50):
            a, b = LM.knn(c["q"], c["t"], nn, "l1"), LM.knn_l1_int(c["q"], c["t"], nn)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            FC.same_tents(LM.match(c, nn, "l1"), LM.match_int(c, nn))
    c = LC.saturating_case()
    d = LM.chain(c["q"], c["t"], "l1")
    assert d[0, 0] == 32640 and d[0, 1] == 32640 and d[0, 2] == 0 and d[1, 2] == 32640 and d[1, 0] == 0
    assert d.max() == 32640


def _scalar_l1(a, b):
    """FLANN's L1<float> on one pair, dim % 4 == 0, one np.float32 operation at a time"""
    r = np.float32(0)
    for k in range(0, len(a), 4):
        e = [np.float32(a[k + i] - b[k + i]) for i in range(4)]
        r = np.float32(r + np.float32(np.float32(np.float32(abs(e[0]) + abs(e[1])) + abs(e[2])) + abs(e[3])))
    return r


def test_the_l1_chain_on_float_rows_is_the_scalar_loop_and_no_other_order(modsx):
    rs = np.random.RandomState(3)
    other_differs = {"knn_f64_rounded_once": False, "knn_f32_left_to_right": False}
    for name, c in _cases():
        if name in ("integer", "walk_l1_int", "saturating"):
            continue
        q, t = c["q"], c["t"]
        d = LM.chain(q, t, "l1")
        for _ in range(200):
            i, j = rs.randint(len(q)), rs.randint(len(t))
            assert d[i, j].view(np.uint32) == _scalar_l1(q[i], t[j]).view(np.uint32), (name, i, j)
        ref = LM.match(c, 50, "l1")
        for other in (LC.knn_f64_rounded_once, LC.knn_f32_left_to_right):
            idx, dist = other(q, t, 50)
            mi, md = LM.knn(q, t, 50, "l1")
            rows, _ = FC.walk(idx, dist, c["pos"], c["ratio"], c["cd"], 50)
            if not np.array_equal(idx, mi) or not np.array_equal(dist.view(np.uint32), md.view(np.uint32)) or _differs(LM.tents(rows), ref):
                other_differs[other.__name__] = True
    assert all(other_differs.values()), other_differs


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("nn", [2, 4, 50])
def test_walk_case_reaches_every_end(modsx, nn, integer):
    c = LC.walk_case(integer=integer)
    assert set(c["expect"].values()) == set(LC.EXPECT_ENDS) == set(LC.EXPECT_STAGE_NN50)
    if integer:
        assert np.array_equal(c["q"], np.round(c["q"])) and c["q"].min() >= 0 and c["q"].max() <= 255
        assert np.array_equal(c["t"], np.round(c["t"])) and c["t"].min() >= 0 and c["t"].max() <= 255
    idx, dist = LM.knn(c["q"], c["t"], nn, "l1")
    _, ends = FC.walk(idx, dist, c["pos"], c["ratio"], c["cd"], nn)
    for q, name in c["expect"].items():
        assert ends[q] == LC.EXPECT_ENDS[name][nn], (name, nn, ends[q])
    ia, da = LM.knn(c["q"], c["t"], len(c["t"]), "l1")
    stage = FC.expected_stage(ia, da, c["pos"], c["ratio"], c["cd"], nn)
    for q, name in c["expect"].items():
        assert stage[q] == (LC.EXPECT_STAGE_NN50[name] if nn == 50 else 0), (name, nn)
    if not integer:
        # the distances are the planted numbers themselves
        q = {v: k for k, v in c["expect"].items()}["record_j3"]
        assert [float(x) for x in da[q, :4]] == [float(np.float32(x)) for x in (1, 1.2, 1.3, 4)]


def test_threshold_case_sits_on_the_threshold(modsx):
    c = LC.threshold_case()
    assert c["ratio"] ** 2 == 0.25
    idx, dist = LM.knn(c["q"], c["t"], 50, "l1")
    _, ends = FC.walk(idx, dist, c["pos"], c["ratio"], c["cd"], 50)
    byname = {v: k for k, v in c["expect"].items()}
    one, four = np.float32(1), np.float32(4)
    q = byname["exact"]
    assert dist[q, 0] == one and dist[q, 1] == four and float(dist[q, 0] / dist[q, 1]) == 0.25 and ends[q] == ("record", 1)
    q = byname["divisor_up"]
    assert dist[q, 0] == one and dist[q, 1] == np.nextafter(four, np.float32(5)) and float(dist[q, 0] / dist[q, 1]) < 0.25
    assert ends[q] == ("record", 1)
    q = byname["dividend_up"]
    assert dist[q, 0] == np.nextafter(one, np.float32(2)) and dist[q, 1] == four and float(dist[q, 0] / dist[q, 1]) > 0.25
    assert ends[q] == ("record", 2)


def test_subnormal_case_depends_on_subnormals(modsx):
    c = LC.subnormal_case()
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(c["q"]) < tiny).all() and (np.abs(c["t"]) < tiny).all()          # the inputs themselves
    e = c["q"][:, None, :] - c["t"][None, :, :]
    assert (np.abs(e) < tiny).all() and (e != 0).mean() > 0.99
    idx, dist = LM.knn(c["q"], c["t"], 50, "l1")
    assert (dist < tiny).all() and (dist[:, 1] > 0).all()
    assert not np.array_equal(idx[:, 0], np.zeros(len(idx), np.int32))              # flushed to zero, train 0 would win everywhere
    assert len(LM.match(c, 50, "l1")) > 10


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("splits", [0, 1, 2, 3, 1 << 20])
def test_tie_case_straddles_tile_and_split_edges(modsx, splits, integer):
    n1, dim = 70, 128
    geometry = (lambda a, b, s=0: modsx.fginn_l1_geometry(a, b, s)) if integer else (lambda a, b, s=0: modsx.fginn32_geometry(a, b, dim, s))
    T = geometry(n1, 1000)["tile"]
    geo = geometry(n1, LC.TIE_TILES * T - 2, splits)
    assert geo["tiles"] == LC.TIE_TILES
    c = LC.tie_case(geo, n1, dim, integer=integer)
    idx, dist = LM.knn(c["q"], c["t"], 50, "l1")
    _, ends = FC.walk(idx, dist, c["pos"], c["ratio"], c["cd"], 50)
    ref = LM.match(c, 50, "l1")
    tps = geo["tiles_per_split"]
    for qi, (a, b) in enumerate(c["pairs"]):
        assert idx[qi, 0] == a and idx[qi, 1] == b and dist[qi, 0] == dist[qi, 1] > 0      # the lower index first
        r = ref[ref["q"] == qi][0]
        assert (r["t0"], r["t1"]) == (a, b) and r["tj"] not in (a, b) and ends[qi] == ("record", 2)
    a, b = c["pairs"][0]
    assert a // T + 1 == b // T
    a, b = c["pairs"][1]
    assert a // T + 1 == b // T
    if geo["splits"] > 1:
        assert (a // T) // tps + 1 == (b // T) // tps
    a, b = c["pairs"][2]
    assert a == 0 and (b // T) // tps == geo["splits"] - 1


def test_l1_and_l2_tentative_lists_differ(modsx):
    """a device that ran L2 where L1 was asked cannot pass"""
    for c in (FC.random_case(257, 99, 128, 107), FC.random_case(64, 200, 36, 11), FC.integer_case(300, 700, 13)):
        a, b = LM.match(c, 50, "l1"), LM.match(c, 50, "l2")
        assert len(a) > 10 and len(b) > 10
        assert _differs(a, b)
        assert not np.array_equal(LM.knn(c["q"], c["t"], 4, "l1")[1], LM.knn(c["q"], c["t"], 4, "l2")[1])
