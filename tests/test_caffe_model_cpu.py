"""CPU: tests/caffe_model.py is tied to the reference -- its samples to the compiled interpolate (oracle/_ref), its norms to what
the reference's L2normalize / L1normalize / RootNormalize computed on the case rows (tests/golden/caffe_norm_ref.npz, recorded by
tools/make_caffe_norm_fixture.py) -- and the cases of tests/caffe_cases.py reach what they claim to reach."""
import os

import numpy as np
import pytest

import caffe_cases as Cs
import caffe_model as M
from conftest import ROOT


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions differ")
    assert not ((u32(got) != u32(ref)) & ~nan).any(), (what, int(((u32(got) != u32(ref)) & ~nan).sum()))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "caffe_norm_ref.npz"))


@pytest.mark.parametrize("P", Cs.PATCH_SIZES)
def test_samples_equal_the_compiled_interpolate(oracle, P):
    if not oracle.ref_hessaff_available():
        pytest.skip("oracle/_ref/libhessaff_ref.so is not built (the reference's sources are not here)")
    ref = lambda img, *a: oracle.ref_interpolate(img, *(float(x) for x in a[:6]), *a[6:])      # noqa: E731
    for name in Cs.IMAGES:
        regs = Cs.regions(name, P)
        j = M.jobs(regs, Cs.MR_SIZE, P)
        for pl in (Cs.planes(name), (Cs.gray(name),)):
            got, out = M.samples(pl, j, P)
            want, wout = M.samples(pl, j, P, interpolate=ref)
            same_bits(got, want, "%s, P = %d, %d planes" % (name, P, len(pl)))
            assert np.array_equal(out, wout)
        rows, cols = Cs.IMAGES[name]
        t = np.stack([np.full(len(regs), cols, np.float64), np.full(len(regs), rows, np.float64)] + [j[f].astype(np.float64) for f in M.KP] +
                     [np.full(len(regs), P, np.float64)] * 2, 1)
        assert np.array_equal(M.border(j, rows, cols, P), oracle.ref_interpolate_check_borders(t))


@pytest.mark.parametrize("w", Cs.NORM_WIDTHS)
def test_norms_equal_the_recorded_reference(golden, w):
    rows = Cs.norm_rows(w)
    assert np.array_equal(u32(rows), u32(golden["in_%d" % w])), "the fixture was recorded on other rows: run tools/make_caffe_norm_fixture.py"
    for norm in Cs.NORMS:
        same_bits(M.norm_rows(rows, norm), golden["%s_%d" % (Cs.NORM_NAMES[norm], w)], "norm %d at width %d" % (norm, w))
    same_bits(M.norm_rows(rows, M.NORM_NONE), rows)


def test_region_cases_reach_what_they_claim():
    names = Cs.REGION_NAMES
    for name, (rows, cols) in Cs.IMAGES.items():
        for P in Cs.PATCH_SIZES:
            b, border, outside = Cs.model_bytes(name, True, P)
            k = {n: i for i, n in enumerate(names)}
            what = (name, P)
            assert not outside[~border].any(), what                       # the truncation branch reports nothing
            if P == 41:
                # both branches of interpolate; every border and the corner lose samples; the far region loses all of them
                assert not border[k["inside"]] and not border[k["inside_small"]], what
                for n in ("left", "right", "top", "bottom", "corner", "far_corner", "outside", "larger_than_image"):
                    assert border[k[n]] and outside[k[n]], (what, n)
                for n in ("rotated", "sheared", "anisotropic", "mirrored"):
                    assert not border[k[n]] or name == "b", (what, n)
            assert not b[k["outside"]].any(), what                         # an all-zero patch: the blob is -mean
            j = M.jobs(Cs.regions(name, P), Cs.MR_SIZE, P)
            assert j["curr_sc"][k["tie"]] == 1.0 and j["a11"][k["tie"]] == 1.0 and j["a22"][k["tie"]] == 1.0, what
            # which border each of the four regions crosses: the lost samples are on that side of the patch
            if P >= 3:
                z = lambda n: np.argwhere(b[k[n], 2] == 0)                 # noqa: E731  (R is never 0 inside the image)
                assert (z("left")[:, 1] < P // 2).all() and (z("right")[:, 1] > P // 2).all(), what
                assert (z("top")[:, 0] < P // 2).all() and (z("bottom")[:, 0] > P // 2).all(), what
    assert (Cs.planes("a")[2] > 0.5).all() and (Cs.planes("b")[2] > 0.5).all()


def test_ties_and_clamps_are_reached():
    down = up = low = high = 0
    for name in Cs.IMAGES:
        for P in Cs.PATCH_SIZES:
            regs = Cs.regions(name, P)
            j = M.jobs(regs, Cs.MR_SIZE, P)
            v, _ = M.samples(Cs.planes(name), j, P)
            tie = v[list(Cs.REGION_NAMES).index("tie"), 0]              # the plane of consecutive integers at x = k + 0.5
            half = tie[(tie - np.floor(tie)) == 0.5]
            if P >= 3:
                assert len(half) > 0, (name, P)
            b = M.to_bytes(half)
            down += int((b < half).sum())
            up += int((b > half).sum())
            assert (b % 2 == 0).all()
            low += int((v < -0.5).sum())
            high += int((v > 255.5).sum())
    assert down > 0 and up > 0, (down, up)
    assert low > 0 and high > 0, (low, high)
    assert list(M.to_bytes(np.array([0.5, 1.5, 2.5, -20.0, 300.0, 254.5, 255.5], np.float32))) == [0, 2, 2, 0, 255, 254, 255]
    assert min(p.min() for p in Cs.planes("a")) == -20.0 and max(p.max() for p in Cs.planes("a")) == 300.0
    assert Cs.gray("a").min() == -20.0 and Cs.gray("a").max() == 300.0


def test_means_truncate_toward_zero():
    b = np.zeros((1, 3, 1, 1), np.uint8)
    assert list(M.blob(b, Cs.MEANS[1]).reshape(-1)) == [-104.0, 3.0, 0.0]       # 104.9 -> 104, -3.7 -> -3, 0.5 -> 0
    assert list(M.blob(b + 7, Cs.MEANS[2]).reshape(-1)) == [7.0, 7.0, 7.0]


@pytest.mark.parametrize("norm", Cs.NORMS)
def test_another_summation_order_gives_other_bits(norm):
    """the planted rows tell the reference's chain from a reversed one and from a balanced tree"""
    planted = "absorb_l2" if norm == M.NORM_L2 else "cancel"
    at = Cs.NORM_ROW_NAMES.index(planted)
    for w in Cs.NORM_WIDTHS:
        if w < 63:
            continue                     # fewer than three ones behind the large element change nothing in f64
        row = Cs.norm_rows(w)[at:at + 1]
        want = M.norm_rows(row, norm)
        rev = M.finish_rows(row, norm, M.row_sums(row, norm, order=range(w - 1, -1, -1)))
        tree = M.finish_rows(row, norm, M.pairwise_sums(row, norm))
        for other in (rev, tree):
            nan = np.isnan(want) | np.isnan(other)
            assert ((u32(want) != u32(other)) & ~nan).any() or not np.array_equal(np.isnan(want), np.isnan(other)), (norm, w)


def test_single_element_rows_fall_on_either_side_of_512():
    for w in Cs.NORM_WIDTHS:
        rows = Cs.norm_rows(w)
        k = {n: i for i, n in enumerate(Cs.NORM_ROW_NAMES)}
        l2, l1 = M.norm_rows(rows, M.NORM_L2), M.norm_rows(rows, M.NORM_L1)
        assert l2[k["single_1p1_first"], 0] == 512.0 and l2[k["single_2p3_last"], w - 1] == 511.0
        assert l1[k["single_3_mid"], w // 2] == 512.0 and l1[k["single_49_first"], 0] == 511.0
        assert np.isnan(l2[k["zero"]]).all() and np.isnan(l1[k["zero"]]).all()
        root = M.norm_rows(rows, M.NORM_ROOTL2)
        neg = rows[k["negative_entry"]] < 0
        if w > 1:                # a lone negative element is divided by itself
            assert neg.sum() == 1 and np.array_equal(np.isnan(root[k["negative_entry"]]), neg)
        assert M.row_sums(rows[k["zero_sum"]:k["zero_sum"] + 1], M.NORM_L1)[0] == 0.0
        assert not np.isfinite(l1[k["zero_sum"]]).any()
