"""CPU: tests/fginn_db_model.py (the numpy restatement of MatchFlannFGINNPlusDB, matching.cpp:462-572) against the oracle's
MatchFlannFGINN, and the filter formulation the device matcher uses against the direct restatement."""
import numpy as np

from common import oracle_features
import fginn_db_model as M


def _real(oracle, small_pair):
    a, b, _ = small_pair
    _, _, d1 = oracle_features(oracle, a)
    _, r2, d2 = oracle_features(oracle, b)
    return d1, d2, np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)


def test_model_without_database_is_the_oracles_matcher(oracle, small_pair):
    d1, d2, pos2 = _real(oracle, small_pair)
    for ratio, cd, nn in ((0.8, 30.0, 50), (0.9, 10.0, 50), (0.6, 3.0, 50), (1.0, 30.0, 50), (1.3, 5.0, 20)):
        ref = oracle.match_fginn(d1, d2, pos2, ratio, cd, nn)
        got, _ = M.match_fginn_db(d1, d2, pos2, None, ratio, cd, nn)
        assert len(ref) > 5
        M.same_tents(got, ref)


def test_far_database_changes_only_the_ratio(oracle, small_pair):
    """every database row far from every query: ratioDB is far below ratio^2, so the records are the oracle's field for field --
    except `ratio`, which is sqrt(max(r_j, ratioDB)) and therefore at least as large"""
    d1, d2, pos2 = _real(oracle, small_pair)
    d1 = np.minimum(d1, 120).astype(np.float32)
    d2 = np.minimum(d2, 120).astype(np.float32)
    rs = np.random.RandomState(3)
    db = rs.randint(200, 256, (500, 128)).astype(np.float32)       # >= 80 away in every one of the 128 dimensions
    ddb = M.db_nearest(d1, db)
    for ratio, cd in ((0.8, 30.0), (0.9, 10.0)):
        ref = oracle.match_fginn(d1, d2, pos2, ratio, cd)
        got, d2db = M.match_fginn_db(d1, d2, pos2, db, ratio, cd)
        assert len(ref) > 5 and len(got) == len(ref)
        assert (ddb > 128 * 80 * 80 - 1).all()
        for f in M.TENT.names:
            if f != "ratio":
                assert np.array_equal(got[f], ref[f]), f
        with np.errstate(divide="ignore", invalid="ignore"):
            rj = (ref["d1"].astype(np.float32) / ref["d2"].astype(np.float32)).astype(np.float64)
            rdb = (ref["d1"].astype(np.float32) / ddb[ref["q"]]).astype(np.float64)
        assert (got["ratio"] >= ref["ratio"]).all()
        assert np.array_equal(got["ratio"], np.sqrt(np.maximum(rj, rdb)))
        assert np.array_equal(d2db, ddb[ref["q"]].astype(np.float64))


def test_all_points_branch_ignores_the_database(oracle, small_pair):
    d1, d2, pos2 = _real(oracle, small_pair)
    db = M.background_descriptors(oracle, seeds=(11,))
    for ratio, cd, nn in ((1.0, 30.0, 50), (1.3, 5.0, 20)):
        ref = oracle.match_fginn(d1, d2, pos2, ratio, cd, nn)
        got, d2db = M.match_fginn_db(d1, d2, pos2, db, ratio, cd, nn)
        assert len(ref) == len(d1)
        M.same_tents(got, ref)
        assert np.array_equal(d2db, M.db_nearest(d1, db)[ref["q"]].astype(np.float64))


def test_filter_formulation_equals_the_direct_restatement_on_the_planted_input(oracle, small_pair):
    P = M.planted_input(oracle, small_pair)
    ddb = M.db_nearest(P["d1"], P["db"])
    assert ddb[P["q_nan"]] == 0 and ddb[P["q_inf"]] == 0
    for ratio, cd in ((0.8, 30.0), (0.9, 30.0), (0.6, 3.0), (1.0, 30.0)):
        plain = oracle.match_fginn(P["d1"], P["d2"], P["pos2"], ratio, cd)
        direct, dd = M.match_fginn_db(P["d1"], P["d2"], P["pos2"], P["db"], ratio, cd)
        filt, df = M.filter_plain(plain, ddb, ratio)
        M.same_tents(filt, direct)
        assert np.array_equal(dd, df)
        if ratio == 0.8:
            # the database decides something: it rejects, it keeps, it raises ratios; the planted cases fall as stated
            kept = np.isin(plain["q"], direct["q"])
            assert (~kept).sum() * 5 >= len(plain) and kept.sum() * 5 >= len(plain), (len(plain), kept.sum())
            assert (direct["ratio"] > plain["ratio"][kept]).sum() * 5 >= len(direct)
            assert P["q_nan"] in direct["q"] and P["q_inf"] in plain["q"] and P["q_inf"] not in direct["q"]
            print("plain %d kept %d raised %d" % (len(plain), len(direct), (direct["ratio"] > plain["ratio"][kept]).sum()))
