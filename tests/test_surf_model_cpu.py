"""The SURF model (tests/surf_model.py) against the compiled reference's recorded results (tests/golden/surf_ref.npz, written by
tools/make_surf_fixture.py), the library's host tables against the model's and the fixture's, the claims of tests/surf_cases.py,
and two experiments that show an ordering error cannot pass."""
import os

import numpy as np
import pytest

import mods_amd
import surf_cases as Cs
import surf_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surf_ref.npz")
FINITE_MR = tuple(mr for mr in Cs.MR_SIZES if mr not in Cs.MR_NAN)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert [str(n) for n in g["names"]] == Cs.names(), "the fixture is not of this case list: rerun tools/make_surf_fixture.py"
    assert tuple(float(v) for v in g["mr_sizes"]) == Cs.MR_SIZES
    return g


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_rows(got, ref, what):
    """bit for bit, entries that are NaN compared by position"""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.nonzero(((u32(got) != u32(ref)) & ~nan).any(1))[0]
    assert len(bad) == 0, (what, [Cs.names()[i] for i in bad[:10]])


def test_case_list():
    names = Cs.names()
    assert 35 <= len(names) <= 45 and len(set(names)) == len(names)
    p = Cs.patches()
    assert p.shape == (len(names), 41, 41) and p.dtype == np.float32 and np.isfinite(p).all()
    assert p.min() >= 0.0 and p.max() <= 255.0
    assert Cs.MR_SIZES == (5.1962, 20.5, 16.4, 30.0, 100.0)


def test_model_equals_reference_bit_for_bit(golden):
    for m, mr in enumerate(Cs.MR_SIZES):
        same_rows(Cs.model(mr), golden["desc_%d" % m], "mrSize %g" % mr)
        I = Cs.info(mr)["I"][golden["integral_of"]]                # noqa: E741
        assert np.array_equal(u32(I), u32(golden["integral_%d" % m])), mr
    assert [Cs.names()[i] for i in golden["integral_of"]] == list(Cs.INTEGRAL_OF)


def test_tables(golden):
    for m, mr in enumerate(Cs.MR_SIZES):
        model, lib = M.tables(mr), mods_amd.surf_tables(mr)
        for key in ("sample_x", "sample_y"):
            gold = golden["%s_%d" % (key, m)]
            assert np.array_equal(model[key], gold) and np.array_equal(lib[key], gold), (mr, key)
        for key in ("w1", "w2"):
            gold = golden["%s_%d" % (key, m)]
            assert np.array_equal(u32(model[key]), u32(gold)) and np.array_equal(u32(lib[key]), u32(gold)), (mr, key)
        assert model["haar_size"] == lib["haar_size"] == int(golden["haar_size_%d" % m][0]), mr
    t = M.tables(5.1962)
    assert abs(float(t["scale"]) - 7.89) < 0.005 and t["haar_size"] == 16 and (t["x"], t["y"]) == (21, 21)
    assert t["sample_x"][0] < -70 and t["sample_x"][-1] > 41 + 60                # the window reaches far beyond the patch
    assert float(M.tables(20.5)["scale"]) == 2.0 and M.tables(20.5)["haar_size"] == 4
    assert float(M.tables(16.4)["scale"]) == 2.5 and M.tables(16.4)["haar_size"] == 6          # fRound(2.5) = 3
    assert M.tables(30.0)["haar_size"] == 2 and M.tables(100.0)["haar_size"] == 0


def test_rounding_ties_are_reached_at_16p4():
    assert M.tables(16.4)["ties"] > 1000          # k * 2.5 ends in .5 for every odd k, and so does the scale itself
    assert M.fround(np.float32(2.5)) == (3, True) and M.fround(np.float32(-2.5)) == (-2, True)
    assert M.fround(np.float32(20.5)) == (21, True) and M.fround(np.float32(2.4)) == (2, False)
    for mr in (5.1962, 20.5, 30.0):               # elsewhere only the point itself (x = y = fRound(20.5f)) ties
        assert M.tables(mr)["ties"] == 1, mr


def test_a_box_sum_is_negative_before_the_clamp():
    """the clamp of BoxIntegral is live at every mrSize that gives finite rows"""
    bright = set()
    for mr in FINITE_MR:
        lo = Cs.info(mr)["pre_clamp_min"]
        assert (lo < 0).any(), mr
        if any(n.startswith("bright_") and v < 0 for n, v in zip(Cs.names(), lo)):
            bright.add(mr)
    # the bright patches were made for it: beyond the far border at the default mrSize, inside the holes where every box is
    # inside the patch (30.0: without the holes no case is negative there)
    assert {5.1962, 30.0} <= bright, bright
    lo = Cs.info(30.0)["pre_clamp_min"]
    assert all(n.startswith("bright_holes_") for n, v in zip(Cs.names(), lo) if v < 0)


def test_every_index_clamp_of_box_integral_is_taken_on_each_side():
    """min(., 41) bites (an index beyond the far border) and the index is negative (before the near border), for each of r1, c1,
    r2, c2, over the boxes of the default mrSize and of 20.5; at 30.0 every box lies inside the patch"""
    for mr in (5.1962, 20.5):
        a = M.box_args(M.tables(mr)).reshape(-1, 4)
        row, col, rows, cols = a.T
        for name, v in (("r1", row), ("c1", col), ("r2", row + rows), ("c2", col + cols)):
            assert (v > 41).any(), (mr, name, "far side")
            assert (np.minimum(v, 41) - 1 < 0).any(), (mr, name, "near side")
    a = M.box_args(M.tables(30.0)).reshape(-1, 4)
    assert a[:, :2].min() >= 1 and (a[:, 0] + a[:, 2]).max() <= 41 and (a[:, 1] + a[:, 3]).max() <= 41


def test_zero_entries_at_the_default_mr_size():
    """scale 7.89: the samples of the outer sub-regions lie wholly outside the patch and contribute +0.  28 entries are zero in
    every case; a patch with a response everywhere the window allows one (random, levels, region, bright, step, constant) has
    exactly those zero; the single-pixel and single-blob patches have them and more; the patch of zeros is NaN"""
    d = Cs.model(5.1962)
    dense = ("random_", "levels_", "region_", "bright_", "step_", "constant", "saturated")
    sets = {}
    for name, row in zip(Cs.names(), d):
        if np.isnan(row).any():
            assert name == "zero" and np.isnan(row).all()
            continue
        sets[name] = frozenset(np.nonzero(row == 0)[0].tolist())
    structural = sets["random_0"]
    assert len(structural) == 28
    for name, z in sets.items():
        if name.startswith(dense):
            assert z == structural, name
        else:
            assert z > structural, name
    # they are +0, not -0: nothing but x + (+0) ever happens to those sums
    idx = sorted(structural)
    assert all(not u32(row[idx]).any() for name, row in zip(Cs.names(), d) if name != "zero")


def test_cases_reach_what_they_claim():
    names = Cs.names()
    by = dict(Cs.cases())
    assert len(np.unique(by["constant"])) == 1 and not by["zero"].any() and (by["saturated"] == 255.0).all()
    assert len(np.unique(by["step_x"])) == 2 and len(np.unique(by["step_y"])) == 2
    assert (by["step_x"][0] == by["step_x"]).all() and (by["step_y"][:, :1] == by["step_y"]).all()
    for n, (r, c) in (("pixel_tl", (0, 0)), ("pixel_tr", (0, 40)), ("pixel_bl", (40, 0)), ("pixel_br", (40, 40)), ("pixel_centre", (20, 20))):
        assert by[n][r, c] == 255.0 and np.count_nonzero(by[n]) == 1, n
    for n in names:
        if n.startswith("bright_flat_"):
            assert by[n].min() >= 250.0 and by[n].max() <= 251.0 and len(np.unique(by[n])) > 1000, n
        if n.startswith("random_"):
            assert len(np.unique(by[n])) > 1600, n
        if n.startswith("levels_"):
            assert (by[n] == np.floor(by[n])).all(), n
        if n.startswith("region_"):
            assert by[n].max() - by[n].min() > 50.0, n               # a real, photonormalised window
    # one_subregion: at 20.5 only the first sub-region answers
    row = Cs.model(20.5)[names.index("one_subregion")]
    assert np.isfinite(row).all() and row[:4].any() and not row[4:].any()
    # the length is zero exactly where the issue says: the patch of zeros everywhere, every patch at fRound(scale) = 0
    for mr in FINITE_MR:
        d = Cs.model(mr)
        nan_rows = np.isnan(d).any(1)
        assert np.array_equal(nan_rows, np.isnan(d).all(1))
        assert nan_rows[names.index("zero")] and not nan_rows[[names.index(n) for n in names if n.startswith(("random_", "region_"))]].any()
    assert np.isnan(Cs.model(100.0)).all()


def _random_rows(d):
    return d[[i for i, n in enumerate(Cs.names()) if n.startswith("random_")]]


def test_a_pairwise_sum_of_the_81_terms_changes_the_random_cases():
    pats = Cs.patches()[[i for i, n in enumerate(Cs.names()) if n.startswith("random_")]]
    for mr in FINITE_MR:
        other = M.describe(pats, mr, pairwise=True)
        ref = _random_rows(Cs.model(mr))
        assert (u32(other) != u32(ref)).any(), mr
        assert np.allclose(other, ref, rtol=0, atol=1e-5)           # the same descriptor up to rounding


def test_integral_columns_before_rows_changes_the_random_cases():
    pats = Cs.patches()[[i for i, n in enumerate(Cs.names()) if n.startswith("random_")]]
    assert (u32(M.integral(pats, columns_first=True)) != u32(M.integral(pats))).any()
    for mr in FINITE_MR:
        other = M.describe(pats, mr, columns_first=True)
        ref = _random_rows(Cs.model(mr))
        assert (u32(other) != u32(ref)).any(), mr
        assert np.allclose(other, ref, rtol=0, atol=1e-3)
