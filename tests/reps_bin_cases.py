"""Inputs and expectations of the binary-class tests (tests/test_reps_bin_cpu.py, tests/test_gpu_reps_bin.py).

Nothing here calls the code under test except through the `modsx` module it is handed; the search reference is
tests/hamming_model.py."""
import ctypes as C

import numpy as np

import hamming_model as HM

# the reference's names (detectors/structures.hpp, descriptors_parameters.hpp) and the library's numbers for them
DETECTORS = {"HessianAffine": 0, "MSER": 3, "ORB": 4, "SURF": 6}
DESCRIPTORS = {"BRISK": 16, "CAFFE": 8, "DAISY": 9, "FREAK": 17, "HalfRootSIFT": 3, "HalfSIFT": 2, "LIOP": 10, "MROGH": 11, "ORB": 18,
               "RootSIFT": 1, "SIFT": 0, "SURF": 12}
U8_TYPES, F32_TYPES, BIN_TYPES = (0, 1, 2, 3), (8, 9, 10, 11, 12), (16, 17, 18)
HES, MSER, ORBDET, SURFDET = 0, 3, 4, 6
BRISK, FREAK, ORB = 16, 17, 18


def holds(det, typ):
    """does a representation have a class for this (detector, descriptor type)?"""
    if typ in U8_TYPES:
        return det in (HES, MSER)
    if typ in F32_TYPES:
        return det in (HES, MSER, SURFDET)
    return typ in BIN_TYPES and det in (HES, MSER, ORBDET, SURFDET)


def name_ranks():
    """{(detector, type): rank of (descriptor name, detector name) in sorted() over all 12 x 4 names}"""
    names = sorted((dn, tn) for dn in DESCRIPTORS for tn in DETECTORS)
    return {(DETECTORS[tn], DESCRIPTORS[dn]): i for i, (dn, tn) in enumerate(names)}


# ---- the geometry of one problem, restated from its documented rule (kernels_hamming.hip header): tiles of 1024 / WK trains, about
# 2048 / (query blocks) splits, at most one per tile, then no empty split
def kernel_width(nbytes):
    W = (nbytes + 3) // 4
    return 1 if W <= 1 else 2 if W <= 2 else 4 if W <= 4 else 8 if W <= 8 else 16


def tile_len(nbytes):
    return 1024 // kernel_width(nbytes)


def single_geometry(n1, n2, nbytes):
    """(tiles, splits, tiles per split) of one problem alone"""
    T = tile_len(nbytes)
    tiles = max(1, -(-n2 // T))
    gx = max(1, -(-n1 // 256))
    S = max(1, min(-(-2048 // gx), tiles))
    tps = -(-tiles // S)
    return tiles, -(-tiles // tps), tps


GEO_N1 = (1, 255, 256, 257, 5000)
GEO_NBYTES = (1, 4, 5, 32, 33, 64)


def geo_sizes(nbytes):
    T = tile_len(nbytes)
    return (0, 2, T - 1, T, T + 1, 2 * T + 3, 40 * T)


def raw_group_geometry(modsx, n1, n2, nbytes, cap=256):
    """one call of the C entry: (count, geometry[4], per_problem[G][3], splits[count][3])"""
    n2 = np.ascontiguousarray(n2, np.int32)
    geo, per, sp = np.zeros(4, np.int32), np.zeros((len(n2), 3), np.int32), np.zeros((cap, 3), np.int32)
    total = modsx.lib().modsx_debug_hamming_group_geometry(int(n1), n2.ctypes.data_as(C.c_void_p), len(n2), int(nbytes),
                                                           geo.ctypes.data_as(C.c_void_p), per.ctypes.data_as(C.c_void_p),
                                                           sp.ctypes.data_as(C.c_void_p), cap)
    assert 0 <= total <= cap, total
    return total, geo, per, sp[:total]


def check_group_geometry(n1, n2, nbytes, total, geo, per, sp):
    """every property the grouped table must have"""
    T = tile_len(nbytes)
    assert tuple(geo) == (T, kernel_width(nbytes), max(1, -(-n1 // 256)), total)
    at = 0
    for g, n in enumerate(n2):
        if n == 0:
            assert tuple(per[g]) == (0, 0, 0)
            continue
        tiles, S, tps = single_geometry(n1, n, nbytes)
        assert tuple(per[g]) == (tiles, S, tps), (n1, n2, nbytes, g, tuple(per[g]), (tiles, S, tps))
        mine = sp[at:at + S]
        assert (mine[:, 0] == g).all()                            # splits come partner by partner
        assert mine[0, 1] == 0 and mine[-1, 2] == tiles           # ... cover the partner's tiles
        assert (mine[1:, 1] == mine[:-1, 2]).all()                # ... exactly once, in order
        assert (mine[:, 2] > mine[:, 1]).all()                    # no split is empty
        assert (mine[:, 2] - mine[:, 1] <= tps).all()
        at += S
    assert at == total


# ---- rows and regions -----------------------------------------------------------------------------------------------------------------
def regs_for(modsx, n, seed=0, spread=900.0):
    rs = np.random.RandomState(1000 + seed)
    r = np.zeros(n, modsx.REGION)
    r["id"] = np.arange(n)
    p = rs.uniform(10, spread, (n, 2))
    for kp in ("reproj_kp", "det_kp"):
        r[kp]["x"], r[kp]["y"] = p[:, 0], p[:, 1]
        r[kp]["a11"] = r[kp]["a22"] = 1
        r[kp]["s"] = 3
    return r


def rows(n, nbytes, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, nbytes)).astype(np.uint8)


def nonzero_rows(n, nbytes, seed):
    """no all-zero row: byte 0 of every row has bit 0 set"""
    r = rows(n, nbytes, seed)
    r[:, 0] |= 1
    return r


def planted_pair(modsx, n=500, nbytes=32, seed=5, matched=350, flips=12):
    """n regions per side: `matched` rows of the second side are the first side's with up to `flips` bits flipped, at the first
    side's positions under a homography; the rest is clutter"""
    rs = np.random.RandomState(seed)
    H = np.array([[1.1, 0.05, 20], [-0.03, 0.95, -10], [1e-5, 2e-5, 1]])
    p1 = rs.uniform(20, 900, (n, 2))
    x = np.c_[p1, np.ones(n)] @ H.T
    p2 = x[:, :2] / x[:, 2:] + rs.normal(0, 0.5, (n, 2))
    d1 = rs.randint(0, 256, (n, nbytes)).astype(np.uint8)
    d2 = np.stack([HM.flip(d1[i], rs.choice(8 * nbytes, rs.randint(0, flips + 1), replace=False)) for i in range(n)])
    d2[matched:] = rs.randint(0, 256, (n - matched, nbytes))
    p2[matched:] = rs.uniform(20, 900, (n - matched, 2))
    perm = rs.permutation(n)
    d2, p2 = d2[perm], p2[perm]
    regs = []
    for p, A in ((p1, np.eye(2)), (p2, H[:2, :2])):
        r = np.zeros(n, modsx.REGION)
        r["id"] = np.arange(n)
        for kp in ("reproj_kp", "det_kp"):
            r[kp]["x"], r[kp]["y"] = p[:, 0], p[:, 1]
            r[kp]["a11"], r[kp]["a12"], r[kp]["a21"], r[kp]["a22"] = A[0, 0], A[0, 1], A[1, 0], A[1, 1]
            r[kp]["s"] = 3
        regs.append(r)
    return regs[0], d1, regs[1], np.ascontiguousarray(d2)
