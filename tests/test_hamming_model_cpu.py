"""CPU: tests/hamming_model.py (the numpy restatement of MatchFLANNDistance, matching.cpp:607-666, exact Hamming search) pinned to
the oracle's knn_linear, the inputs of tests/test_gpu_hamming.py checked for what they claim to reach, and the library's host-side
record rule (modsx_hamming_tentatives) against the model's."""
import numpy as np
import pytest

from common import oracle_features, laf_of, need_ref
import hamming_model as M


def _small_pair_bits(oracle, small_pair):
    a, b, _ = small_pair
    _, r1, d1 = oracle_features(oracle, a)
    _, r2, d2 = oracle_features(oracle, b)
    return r1, M.binarise(d1), r2, M.binarise(d2)


def _pin(oracle, b1, b2):
    """on bit vectors the squared L2 distance is the Hamming distance: the oracle's exact 2-NN must be the model's"""
    idx, dist = oracle.knn_linear(np.unpackbits(b1, axis=1), np.unpackbits(b2, axis=1), nn=2)
    nn2 = M.knn2(b1, b2)
    assert np.array_equal(idx, nn2[:, [0, 2]])
    assert np.array_equal(dist, nn2[:, [1, 3]].astype(np.float32))
    assert np.array_equal(M.distances(b1, b2)[np.arange(len(b1)), nn2[:, 0]], nn2[:, 1])
    return nn2


def test_model_is_the_oracles_linear_knn_on_the_small_pair(oracle, small_pair):
    _, b1, _, b2 = _small_pair_bits(oracle, small_pair)
    assert b1.shape[1] == 16 and len(b1) > 100 and len(b2) > 100
    _pin(oracle, b1, b2)


def test_model_is_the_oracles_linear_knn_on_the_tie_heavy_case(oracle):
    q, t = M.tie_heavy()
    assert q.shape == (70, 4) and t.shape == (257, 4)
    nn2 = _pin(oracle, q, t)
    D = M.distances(q, t)
    # every query has its nearest train twice (the copied half), so every first neighbour is a tie broken by index
    assert ((D == nn2[:, 1:2]).sum(1) >= 2).all()
    assert (nn2[:, 0] < nn2[:, 2]).any() and (nn2[:, 1] == nn2[:, 3]).all()


def test_planted_case_reaches_what_the_gpu_tests_claim(oracle, modsx):
    nbytes, n1 = 32, 300
    T =modsx.hamming_geometry(n1, 1000, nbytes)["tile"]
    n2 = 5 * T + 3
    for splits in (1, 2, 3, 7, 1 << 20, 0):
        g = modsx.hamming_geometry(n1, n2, nbytes, splits)
        assert g["tile"] == T and g["W"] == 8
        start = M.last_split_start(T, n2, g["splits"])
        copies = M.copies_for(T, start) if g["splits"] > 1 else [0, T - 1, T]
        q, t, info = M.planted(n1, n2, nbytes, copies)
        nn2 = _pin(oracle, q, t)
        M.check_planted(nn2, info)
        D = M.distances(q, t)
        P = M.PLANT
        assert (D[P["tie_first"]] == 5).sum() == 2 and D[P["tie_first"]].min() == 5              # a first-neighbour tie
        assert (D[P["tie_second"]] == 9).sum() == 2 and np.sort(D[P["tie_second"]])[0] == 3      # a second-neighbour tie
        assert (D[P["nan"]] == 0).sum() == 2
        assert (D[P["copies"]] == 2).sum() == 3
        # the three copies stand in different tiles, and (with more than one split) the last in another split than the first two
        tiles = [c // T for c in info["copies"]]
        assert tiles[0] == 0 and info["copies"][1] == T - 1 and tiles[2] >= 1
        if g["splits"] > 1:
            assert info["copies"][2] == start and start % T == 0 and start // T > tiles[1]
        d1 = nn2[:, 1]
        assert (d1 == M.MAX_DISTANCE).any() and (d1 == M.MAX_DISTANCE + 1).any() and (d1 == 0).any()
    assert modsx.hamming_geometry(n1, n2, nbytes, 1 << 20)["splits"] == 6      # at most one split per tile


def test_record_rule_of_the_library_is_the_models(modsx):
    q, t, _ = M.planted(300, 643, 32, [0, 127, 512])
    cases = [M.knn2(q, t), M.knn2(*M.tie_heavy())]
    for nn2 in cases:
        for thr in (60, 60.9, 0.5, 1e9):
            ref = M.tentatives(nn2, thr)
            got = modsx.hamming_tentatives(nn2, thr)
            assert got.dtype == modsx.TENT
            M.same_tents(got, ref)
        assert len(M.tentatives(nn2, 1e9)) == len(nn2)
        assert np.array_equal(modsx.hamming_tentatives(nn2, 0.5)["d1"], np.zeros((nn2[:, 1] == 0).sum()))
    nn2 = cases[0]
    a, b = modsx.hamming_tentatives(nn2, 60), modsx.hamming_tentatives(nn2, 60.9)
    M.same_tents(a, b)                                          # 60.9 truncates to 60
    assert M.PLANT["at_max"] in a["q"] and M.PLANT["above_max"] not in a["q"]
    assert M.PLANT["above_max"] in modsx.hamming_tentatives(nn2, 61)["q"]
    rec = a[a["q"] == M.PLANT["nan"]]
    assert len(rec) == 1 and rec["d1"][0] == 0 and rec["d2"][0] == 0 and np.isnan(rec["ratio"][0])      # 0 / 0 is returned as NaN
    assert not np.isinf(a["ratio"]).any()
    assert len(modsx.hamming_tentatives(np.zeros((0, 4), np.int32), 60)) == 0
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):      # MODSX_ERR_ARG
            modsx.hamming_tentatives(nn2, bad)
    assert len(modsx.hamming_tentatives(nn2, 60)) == len(a)     # still usable afterwards


def test_small_pair_input_is_fit_for_the_fused_test(oracle, small_pair):
    """threshold 30 on the binarised small_pair descriptors gives a verification problem worth comparing"""
    need_ref(oracle)
    r1, b1, r2, b2 = _small_pair_bits(oracle, small_pair)
    tent = M.match(b1, b2, 30)
    assert not np.isnan(tent["ratio"]).any()
    assert len(tent) >= 100
    pts = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                    r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = oracle.duplicate_filtering(pts, tent["ratio"], 2.0, True)
    sel = order[keep]
    res = oracle.loransac_h(pts[sel], laf_of(r1, tent["q"][sel]), laf_of(r2, tent["t0"][sel]), seed=1)
    print("records %d, after the duplicate filter %d, verified %d" % (len(tent), len(sel), int(res["keep"].sum())))
    assert int(res["keep"].sum()) >= 50
