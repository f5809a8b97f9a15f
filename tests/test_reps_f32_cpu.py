"""CPU: what the float classes of stored representations decide on the host -- the order match_reps concatenates the classes in
(modsx_rep_class_rank) and the train axis of the grouped f32 search (modsx_debug_fginn32_group_geometry)."""
import itertools

import numpy as np
import pytest

# the reference's names: descriptor type -> RegionVectorMap key, detector -> DetectorName
DESC_NAME = {8: "CAFFE", 9: "DAISY", 3: "HalfRootSIFT", 2: "HalfSIFT", 10: "LIOP", 11: "MROGH", 1: "RootSIFT", 0: "SIFT", 12: "SURF"}
DET_NAME = {0: "HessianAffine", 3: "MSER", 6: "SURF"}


def test_class_rank_is_the_string_order_of_the_reference_names(modsx):
    order = sorted((DESC_NAME[t], DET_NAME[d], d, t) for t in DESC_NAME for d in DET_NAME)      # std::map<string, std::map<string, ...>>
    assert len(order) == 27
    for rank, (_, _, d, t) in enumerate(order):
        assert modsx.rep_class_rank(d, t) == rank, (d, t)
    # the SIFT-family classes keep the order they had: types 3, 2, 1, 0 and HessianAffine before MSER inside a type
    old = [(d, t) for t in (3, 2, 1, 0) for d in (0, 3)]
    ranks = [modsx.rep_class_rank(d, t) for d, t in old]
    assert ranks == sorted(ranks) and len(set(ranks)) == 8
    for d in (1, 2, 4, 5, 7, -1):                      # DoG, Harris and numbers that name no detector
        for t in DESC_NAME:
            assert modsx.rep_class_rank(d, t) == -1
    for t in (4, 5, 6, 7, 13, -1):
        for d in DET_NAME:
            assert modsx.rep_class_rank(d, t) == -1


def _check_table(modsx, n1, n2, dim):
    g = modsx.fginn32_group_geometry(n1, n2, dim)
    T = g["tile"]
    assert g["gx"] == (n1 + 255) // 256 and g["DK"] >= dim
    covered = [np.zeros((m + T - 1) // T, np.int32) for m in n2]
    last = (-1, 0)
    for p, t0, t1 in g["splits"]:
        assert 0 <= p < len(n2) and n2[p] > 0            # an empty problem has no split; a split names one problem
        assert 0 <= t0 < t1 <= len(covered[p])           # no split is empty
        assert (p, t0) >= last                           # problems in order, a problem's splits in tile order
        last = (p, t1)
        covered[p][t0:t1] += 1
    for p, m in enumerate(n2):
        assert (covered[p] == 1).all(), (n1, n2, dim, p)  # every tile in exactly one split
        tiles, S, tps = g["per_problem"][p]
        assert tiles == len(covered[p]) and S == sum(1 for s in g["splits"] if s[0] == p)
        assert (m == 0) == (S == 0)
        if m:
            assert (tiles + tps - 1) // tps == S
        if m:                                              # a problem is cut as it is cut alone, whatever shares the launch
            one = modsx.fginn32_geometry(n1, m, dim)
            assert (tiles, S, tps) == (one["tiles"], one["splits"], one["tiles_per_split"])
    return g


@pytest.mark.parametrize("dim", [32, 64, 128, 144, 200, 256])
def test_group_geometry_covers_every_tile_once(modsx, dim):
    T = modsx.fginn32_geometry(1, 1, dim)["tile"]
    sizes = [0, 1, T - 1, T, T + 1, 2 * T + 1, 20011]
    rs = np.random.RandomState(dim)
    for n1 in (1, 255, 256, 257, 5000):
        for m in sizes:                                   # G = 1: the single-problem geometry
            g = _check_table(modsx, n1, [m], dim)
            if m:
                one = modsx.fginn32_geometry(n1, m, dim)
                assert g["per_problem"][0] == (one["tiles"], one["splits"], one["tiles_per_split"])
                assert g["tile"] == one["tile"] and g["DK"] == one["DK"] and len(g["splits"]) == one["splits"]
        for G in (2, 3, 4):
            combos = list(itertools.product(sizes, repeat=G))
            for k in rs.choice(len(combos), 40, replace=False):
                _check_table(modsx, n1, list(combos[k]), dim)
            _check_table(modsx, n1, [0] * G, dim)
            _check_table(modsx, n1, [20011] * G, dim)


def test_group_geometry_cuts_each_problem_as_alone(modsx):
    g = modsx.fginn32_group_geometry(5000, [20011, 2000, 0, 20011], 128)
    S = [p[1] for p in g["per_problem"]]
    assert S[2] == 0 and S[0] == S[3] == modsx.fginn32_geometry(5000, 20011, 128)["splits"] and S[1] == modsx.fginn32_geometry(5000, 2000, 128)["splits"]
    assert len(g["splits"]) == sum(S)


def test_group_geometry_refusals(modsx):
    for bad in ((0, [5], 64), (5, [5] * 5, 64), (5, [], 64), (5, [5], 66), (5, [-1], 64), (5, [5], 260)):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            modsx.fginn32_group_geometry(*bad)
