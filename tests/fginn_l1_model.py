"""A numpy model of the FGINN search under vector_dist = L1 (FLANN's L1<float> as the linear index calls it), for the tests of
kernels_fginn32.hip (MODSX_DIST_L1) and kernels_fginn_l1.hip.  The oracle's knn_linear / match_fginn are L2 only, so this model is
pinned on the CPU first (tests/test_fginn_l1_model_cpu.py): with chain = "l2" it must equal the oracle bit for bit, which pins the
sort, the key, the tie rule and the walk and leaves one line, the chain, unpinned."""
import numpy as np

import fginn32_cases as FC


def chain(q, t, kind):
    """[n1][n2] f32 distances: one f32 chain per pair over k = 0, 4, 8, ...: r = r + (((f(e0) + f(e1)) + f(e2)) + f(e3)) with
    e_i = a[k+i] - b[k+i] and f = |.| ("l1") or the square ("l2"); every operation rounded to f32"""
    assert kind in ("l1", "l2")
    q, t = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
    assert q.shape[1] == t.shape[1] and q.shape[1] % 4 == 0
    d = np.zeros((len(q), len(t)), np.float32)
    for k in range(0, q.shape[1], 4):
        e = q[:, None, k:k + 4] - t[None, :, k:k + 4]                 # f32
        p = np.abs(e) if kind == "l1" else e * e
        d = d + (((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]) + p[:, :, 3])
    return d


def knn(q, t, nn, kind):
    """(idx [n1][nn] i32, -1 = no train; dist [n1][nn] f32): the chain, then neighbours by the key (f32 bits << 32) | train index"""
    return FC._sorted_knn(chain(q, t, kind), nn)


def knn_l1_int(q, t, nn):
    """the same for rows that hold integers, by brute force in int64: no summation order to get wrong"""
    qi, ti = np.asarray(q).astype(np.int64), np.asarray(t).astype(np.int64)
    assert np.array_equal(qi, q) and np.array_equal(ti, t)
    assert qi.shape[1] * (max(np.abs(qi).max(initial=0), np.abs(ti).max(initial=0)) * 2) < 1 << 24      # every sum is exact in f32
    d = np.zeros((len(qi), len(ti)), np.int64)
    for k in range(qi.shape[1]):
        e = qi[:, k, None] - ti[None, :, k]
        np.abs(e, out=e)
        d += e
    return FC._sorted_knn(d.astype(np.float32), nn)


def tents(rows):
    import mods_amd
    return FC.tents_array(rows, mods_amd.TENT)


def match(case, nn, kind, n1=None, n2=None):
    """the tentative records (mods_amd.TENT) of a case: knn, then the reference's walk (fginn32_cases.walk)"""
    q = case["q"] if n1 is None else case["q"][:n1]
    t, pos = (case["t"], case["pos"]) if n2 is None else (case["t"][:n2], case["pos"][:n2])
    idx, dist = knn(q, t, nn, kind)
    rows, _ = FC.walk(idx, dist, pos, case["ratio"], case["cd"], nn)
    return tents(rows)


def match_int(case, nn, n1=None, n2=None):
    """match() for integer rows with knn_l1_int in place of the chain"""
    q = case["q"] if n1 is None else case["q"][:n1]
    t, pos = (case["t"], case["pos"]) if n2 is None else (case["t"][:n2], case["pos"][:n2])
    idx, dist = knn_l1_int(q, t, nn)
    rows, _ = FC.walk(idx, dist, pos, case["ratio"], case["cd"], nn)
    return tents(rows)
