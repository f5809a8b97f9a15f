"""The LIOP model (tests/liop_model.py) against the compiled reference's recorded results (tests/golden/liop_ref.npz, written by
tools/make_liop_fixture.py), the library's host tables against the model's, and the claims of tests/liop_cases.py: which cases
take which path, and that a wrong tie order cannot pass."""
import os

import numpy as np
import pytest

import liop_cases as Cs
import liop_model as M
import mods_amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "liop_ref.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert [str(n) for n in g["names"]] == [n for n, _ in Cs.cases()], "the fixture is not of this case list: rerun tools/make_liop_fixture.py"
    return g


@pytest.fixture(scope="module")
def model():
    return Cs.model()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_model_equals_reference_bit_for_bit(golden, model):
    for (name, _), m, d, perm in zip(Cs.cases(), model, golden["desc"], golden["perm"]):
        assert np.array_equal(u32(m["desc"]), u32(d)), name
        assert np.array_equal(m["perm"], perm.astype(np.int64)), name       # the quicksort replay, tie order included


def test_tables(golden):
    pix, sx, sy = M.tables()
    assert len(pix) == 673 == M.NPIX and M.BIN_AREA == 112 and M.EDGES == (112, 224, 336, 448, 560)
    lp, lsx, lsy = mods_amd.liop_tables()
    for got, ref, gold in ((lp, pix, golden["pixels"]), (lsx, sx, golden["sx"]), (lsy, sy, golden["sy"])):
        assert np.array_equal(np.asarray(got, ref.dtype), ref)
        assert np.array_equal(ref, gold)
    assert u32(golden["intensity_threshold"]) == u32(-M.THRESH)
    assert 0 not in pix                                                       # the x == 0 && y == 0 skip never bites at L = 41


def test_out_of_patch_samples_have_zero_weight():
    """Exactly two samples touch column / row 41, both with a weight of exactly 0: pixel (34, 20) at t = 0 (sx = 40.0, reads the
    next row's column 0) and pixel (20, 34) at t = 0 (sy = 40.0, reads two floats past the patch)."""
    pix, sx, sy = M.tables()
    idx, wx, wy, ix, iy = M._sample_operands()
    touch = [(int(pix[i]) % 41, int(pix[i]) // 41, t) for i in range(M.NPIX) for t in range(4) if ix[i, t] + 1 >= 41 or iy[i, t] + 1 >= 41]
    assert sorted(touch) == [(20, 34, 0), (34, 20, 0)]
    i = int(np.nonzero(pix == 34 + 20 * 41)[0][0])
    assert sx[i, 0] == 40.0 and wx[i, 0] == 0.0 and idx[i, 0, 1] == 41 + 20 * 41
    i = int(np.nonzero(pix == 20 + 34 * 41)[0][0])
    assert sy[i, 0] == 40.0 and wy[i, 0] == 0.0 and list(idx[i, 0, 2:]) == [-1, -1]      # 1681 + 20, 1681 + 21: outside
    assert (ix >= 0).all() and (iy >= 0).all()
    # the value does not depend on what lies there: poison the in-patch operand of the first, nothing else to poison for the second
    p = Cs.cases()[0][1].copy()
    a = M.neighbour_values(p)
    p[21, 0] = np.float32(12345.0)
    i = int(np.nonzero(pix == 34 + 20 * 41)[0][0])
    assert M.neighbour_values(p)[i, 0] == a[i, 0]


def test_paths_are_balanced(model):
    exact = sum(bool(m["straddle"]) for m in model)
    n = len(model)
    assert 3 * exact >= n and 3 * (n - exact) >= n, (exact, n)


def test_cases_reach_what_they_claim(model):
    by = {name: (p, m) for (name, p), m in zip(Cs.cases(), model)}
    meta = Cs.meta()
    seen = set()
    for name, kw in meta.items():
        p, m = by[name]
        if "edges" in kw:
            assert m["straddle"] == tuple(kw["edges"]), name
            seen.update(kw["edges"]) if len(kw["edges"]) == 1 else None
        if kw.get("disc_const"):
            assert len(np.unique(M.keys_of(p) + np.float32(0.0))) == 1 and m["straddle"] == M.EDGES, name
            assert len(np.unique(p)) > 100, name                              # the surround varies
    assert seen == set(M.EDGES)                                               # every edge alone
    assert any(len(kw.get("edges", ())) > 1 for kw in meta.values())          # and several at once
    for name, (p, m) in by.items():
        keys = M.keys_of(p)
        if name.startswith("distinct_"):
            assert len(np.unique(keys)) == M.NPIX and not m["straddle"], name
        if name.startswith("ties_inside_"):
            assert len(np.unique(keys)) < M.NPIX and not m["straddle"], name
        if name.startswith("two_valued_"):
            assert len(np.unique(p)) == 2 and m["straddle"], name
        assert m["ssq"] < 1 << 24, name
    assert (by["saturated_half"][0][:, 21:] == 255.0).all() and (by["saturated_half"][0][:, :21] < 255.0).all()
    assert {0.0, 255.0} <= set(np.unique(by["saturated_2"][0]).tolist())      # clamped at both ends
    assert any(name.startswith("saturated_") and m["straddle"] for name, (p, m) in by.items())
    # the degenerate end of the threshold: a flat disc has threshold 0 and still a histogram, from its surround
    assert by["disc_const_0"][1]["thr"] == 0 and by["disc_const_0"][1]["ssq"] > 0


def test_every_straddle_case_differs_under_a_stable_sort(model):
    """a sort that orders equal intensities by index gives another descriptor wherever a tie group lies across a cut"""
    n = 0
    for (name, p), m in zip(Cs.cases(), model):
        stable = M.process(p, perm=M.stable_perm(p))
        if m["straddle"]:
            assert not np.array_equal(stable["desc"], m["desc"]), name
            n += 1
        else:
            assert np.array_equal(u32(stable["desc"]), u32(m["desc"])), name  # no straddle: any sort by key is the reference's
    assert n >= 20


def test_neighbour_ties_with_weight(model):
    """two of the four neighbour samples equal while the pixel's weight is not 0: permIndex depends on the 4-sort's tie order"""
    hit = 0
    for m in model:
        tied = np.array([len(set(r.tolist())) < 4 for r in m["nv"]])
        hit += int((tied & (m["weight"] > 0)).sum())
    assert hit > 1000


def test_threshold_pair(model):
    """thr_lo / thr_hi: one neighbour pair sits within one f32 ulp of the threshold, on either side"""
    by = {name: m for (name, _), m in zip(Cs.cases(), model)}
    i, k, t = Cs.meta()["thr_lo"]["threshold_pair"]
    lo, hi = by["thr_lo"], by["thr_hi"]
    assert lo["thr"] == hi["thr"] and lo["thr"] > 0
    thr = float(lo["thr"])
    a_lo, a_hi, b = lo["nv"][i, k], hi["nv"][i, k], lo["nv"][i, t]
    assert hi["nv"][i, t] == b
    assert not float(a_lo) > float(b) + thr and float(np.nextafter(a_lo, np.float32(np.inf))) > float(b) + thr
    assert float(a_hi) > float(b) + thr and not float(np.nextafter(a_hi, np.float32(-np.inf))) > float(b) + thr
    assert hi["weight"][i] == lo["weight"][i] + 1
    assert not np.array_equal(lo["desc"], hi["desc"])
