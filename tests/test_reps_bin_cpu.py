"""CPU: the class order over every kind of class of a stored representation (modsx_rep_class_order) and the table of the grouped
Hamming launch set (modsx_debug_hamming_group_geometry), host functions of their arguments."""
import itertools

import reps_bin_cases as BC


def test_class_order_is_the_rank_of_the_names_over_all_descriptors_and_detectors(modsx):
    ranks = BC.name_ranks()
    assert len(ranks) == 48 and sorted(ranks.values()) == list(range(48))
    held = 0
    for (det, typ), want in ranks.items():
        if BC.holds(det, typ):
            assert modsx.rep_class_order(det, typ) == want, (det, typ)
            held += 1
        else:
            assert modsx.rep_class_order(det, typ) == -1, (det, typ)      # e.g. ORB x SIFT: a pair that names no class
    assert held == 8 + 15 + 12
    # BRISK sorts in front of CAFFE, FREAK between DAISY and HalfRootSIFT, ORB between MROGH and RootSIFT; the ORB detector
    # between MSER and SURF
    assert modsx.rep_class_order(BC.HES, BC.BRISK) == 0 and modsx.rep_class_order(BC.SURFDET, 12) == 47
    assert modsx.rep_class_order(BC.MSER, BC.ORB) < modsx.rep_class_order(BC.ORBDET, BC.ORB) < modsx.rep_class_order(BC.SURFDET, BC.ORB)
    assert modsx.rep_class_order(BC.SURFDET, 11) < modsx.rep_class_order(BC.HES, BC.ORB) < modsx.rep_class_order(BC.HES, 1)


def test_class_order_refuses_what_names_no_class(modsx):
    for typ in list(BC.U8_TYPES) + list(BC.F32_TYPES) + list(BC.BIN_TYPES):
        for det in (1, 2, 5, 7, -1, -4, 100):                     # DoG, Harris, numbers that name no detector
            assert modsx.rep_class_order(det, typ) == -1, (det, typ)
    for det in (BC.HES, BC.MSER, BC.ORBDET, BC.SURFDET):
        for typ in (4, 5, 6, 7, 13, 14, 15, 19, -1, -16, 1000):
            assert modsx.rep_class_order(det, typ) == -1, (det, typ)


def test_class_order_agrees_with_class_rank_on_the_classes_rank_knows(modsx):
    known = [(d, t) for d in (BC.HES, BC.MSER, BC.SURFDET) for t in list(BC.U8_TYPES) + list(BC.F32_TYPES)]
    assert len(known) == 27 and all(modsx.rep_class_rank(d, t) >= 0 for d, t in known)
    # rank counts three detectors for every descriptor (SIFT-family x SURF included); order is -1 where no class exists
    have = [k for k in known if modsx.rep_class_order(*k) >= 0]
    assert len(have) == 23
    assert sorted(have, key=lambda k: modsx.rep_class_rank(*k)) == sorted(have, key=lambda k: modsx.rep_class_order(*k))
    # the values of rep_class_rank are what they were, and it does not know the new classes
    assert [modsx.rep_class_rank(BC.HES, t) for t in (8, 9, 3, 2, 10, 11, 1, 0, 12)] == list(range(0, 27, 3))
    for det in (BC.HES, BC.MSER, BC.ORBDET, BC.SURFDET):
        for typ in BC.BIN_TYPES:
            assert modsx.rep_class_rank(det, typ) == -1
    assert modsx.rep_class_rank(BC.ORBDET, 1) == -1


def test_single_problem_rule_restated_here_equals_the_single_problem_entry(modsx):
    for n1 in BC.GEO_N1:
        for nbytes in BC.GEO_NBYTES:
            for n2 in BC.geo_sizes(nbytes):
                if n2 == 0:
                    continue
                g = modsx.hamming_geometry(n1, n2, nbytes)
                tiles, S, tps = BC.single_geometry(n1, n2, nbytes)
                assert (g["tile"], g["splits"], g["workgroups"]) == (BC.tile_len(nbytes), S, S * max(1, -(-n1 // 256))), (n1, n2, nbytes)


def test_group_geometry_cuts_every_partner_as_it_is_cut_alone(modsx):
    combos = 0
    for n1 in BC.GEO_N1:
        for nbytes in BC.GEO_NBYTES:
            sizes = BC.geo_sizes(nbytes)
            for G in (1, 2, 3, 4):
                for n2 in itertools.product(sizes, repeat=G):
                    total, geo, per, sp = BC.raw_group_geometry(modsx, n1, n2, nbytes)
                    BC.check_group_geometry(n1, n2, nbytes, total, geo, per, sp)
                    combos += 1
    assert combos == 5 * 6 * (7 + 49 + 343 + 2401)
    # the Python wrapper hands out the same table; several splits per partner at 5 000 queries against 40 tiles
    g = modsx.hamming_group_geometry(5000, [40 * 32, 0, 35], 64)
    assert g["tile"] == 64 and g["WK"] == 16 and g["gx"] == 20
    assert g["per_problem"] == [BC.single_geometry(5000, 1280, 64), (0, 0, 0), BC.single_geometry(5000, 35, 64)]
    assert g["per_problem"][0][1] > 1 and [s[0] for s in g["splits"]] == [0] * g["per_problem"][0][1] + [2]


def test_group_geometry_refusals(modsx):
    L = modsx.lib()
    import ctypes as C
    import numpy as np
    n2 = np.array([5, 5, 5, 5, 5], np.int32)
    geo, per = np.zeros(4, np.int32), np.zeros((5, 3), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.modsx_debug_hamming_group_geometry(10, p(n2), 0, 32, p(geo), p(per), None, 0) == -1      # G outside 1..4
    assert L.modsx_debug_hamming_group_geometry(10, p(n2), 5, 32, p(geo), p(per), None, 0) == -1
    assert L.modsx_debug_hamming_group_geometry(10, p(n2), 2, 0, p(geo), p(per), None, 0) == -1       # nbytes outside 1..64
    assert L.modsx_debug_hamming_group_geometry(10, p(n2), 2, 65, p(geo), p(per), None, 0) == -1
    one = np.array([5, 1], np.int32)
    assert L.modsx_debug_hamming_group_geometry(10, p(one), 2, 32, p(geo), p(per), None, 0) == -1     # a train class of one region
    assert L.modsx_debug_hamming_group_geometry(10, p(n2), 2, 32, p(geo), p(per), None, 0) == 2
