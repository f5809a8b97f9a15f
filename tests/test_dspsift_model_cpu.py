"""The DSP-SIFT model (tests/dspsift_model.py) against the compiled reference's recorded results (tests/golden/dspsift_ref.npz,
written by tools/make_dspsift_fixture.py) and against the oracle's SIFT classes, and the claims of tests/dspsift_cases.py: which
rows clip, that the pooling order and the order of the length sum both matter, on which side of the rounding the ulp pairs fall."""
import os

import numpy as np
import pytest

import dspsift_cases as Cs
import dspsift_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dspsift_ref.npz")
f32, f64 = np.float32, np.float64


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    again = "the fixture is not of this case list: rerun tools/make_dspsift_fixture.py"
    assert [str(n) for n in g["patch_names"]] == Cs.patch_names(), again
    assert [str(n) for n in g["row_names"]] == [n for n, _ in Cs.norm_rows()], again
    assert list(g["max_bins"]) == list(Cs.MAX_BINS), again
    return g


def test_raw_histograms_equal_the_reference_bit_for_bit(golden):
    got = Cs.model_raw()
    assert got.shape == golden["raw"].shape == (len(Cs.patches()), 128)
    for name, a, b in zip(Cs.patch_names(), got, golden["raw"]):
        assert np.array_equal(u32(a), u32(b)), name
    # a patch whose gradients vanish (subnormal values: the squares underflow) gives a histogram of zeros; it is in the list
    empty = [n for n, h in zip(Cs.patch_names(), got) if not h.any()]
    assert len(got) >= 54 + 20 and 1 <= len(empty) <= 3, empty


def test_f32_norm_equals_the_reference_bit_for_bit(golden):
    rows = Cs.norm_row_array()
    for mb, ref in zip(Cs.MAX_BINS, golden["norm"]):
        got = M.sift_norm_f32(rows, mb)
        for (name, _), a, b in zip(Cs.norm_rows(), got, ref):
            assert np.array_equal(u32(a), u32(b.astype(f32))), (name, mb)
    assert Cs.MAX_BINS[0] != Cs.MAX_BINS[1]
    # the two clips differ in whether a value of exactly (float)0.2 starts a second normalisation
    i = [n for n, _ in Cs.norm_rows()].index("exactly_0p2f")
    flags = []
    for mb in Cs.MAX_BINS:
        info = {}
        M.sift_norm_f32(rows[i], mb, info=info)
        flags.append(bool(info["clipped"][0]))
    assert flags == [True, False]


def test_histogram_through_the_f64_norms_equals_the_oracle(oracle):
    """the same vec[128] feeds the four classes of modsx_describe_regions: the model's histogram, put through a restatement of
    the f64 norms, is what the oracle gives for the patch"""
    for name, p in zip(Cs.patch_names(), Cs.patches()):
        vec = M.histogram_f64(p)
        for t in range(4):
            want = oracle.describe_patch(p, photo_norm=0, rootsift=t)[0]
            assert np.array_equal(M.describe_f64(vec, t), want), (name, t)


def test_model_parts():
    b0, b1, w0, w1 = M.bins_and_weights()
    # step = 5 / 40: xi = i // 8, weights multiples of 1 / 8; the frame's bins are clamped with weight 0
    assert list(b1 // 8) == [min(i // 8, 3) for i in range(41)] and list(b0 // 8) == [min(max(i // 8 - 1, 0), 3) for i in range(41)]
    i = np.arange(41)
    assert np.array_equal(w1 * 8, np.where(i < 32, i % 8, 0))                 # bin1 = 4 from column 32 on: clamped, weight 0
    assert np.array_equal(w0 * 8, np.where((i >= 8) & (i < 40), 8 - i % 8, 0))
    m = M.mask()
    assert m[20, 20] == 1 and int((m > 0).sum()) == int(((np.mgrid[-20:21, -20:21] ** 2).sum(0) < 400).sum()) and m[0, 20] == 0 and m[1, 20] > 0


def test_rows_reach_what_they_claim():
    rows = dict(Cs.norm_rows())
    info = {}
    out = M.sift_norm_f32(Cs.norm_row_array(), 0.2, info=info)
    by = {n: (o, c, t) for (n, _), o, c, t in zip(Cs.norm_rows(), out, info["clipped"], info["t"])}
    assert not by["zero"][0].any() and np.isnan(by["zero"][2]).all() and not by["zero"][1]
    o, c, _ = by["one_bin"]
    assert c and o[37] == 255 and o.sum() == 255                              # 1 -> 0.2 -> 1 again
    o, c, _ = by["flat"]
    assert not c and (o == int(512.0 / np.sqrt(128.0) + 0.5)).all()
    assert sum(bool(v[1]) for v in by.values()) >= 10 and sum(not v[1] for v in by.values()) >= 10
    # the ulp pairs: one bit apart in one bin, outputs b and b + 1, 512 v within one f32 ulp of b + 0.5 on either side
    for k, bin_ in enumerate((5, 64, 127)):
        lo, hi = rows["half_lo_%d" % k], rows["half_hi_%d" % k]
        diff = np.nonzero(u32(lo) != u32(hi))[0]
        assert list(diff) == [bin_] and int(u32(hi)[bin_]) - int(u32(lo)[bin_]) == 1
        (olo, clo, tlo), (ohi, chi, thi) = by["half_lo_%d" % k], by["half_hi_%d" % k]
        assert not clo and not chi
        b = int(olo[bin_])
        assert int(ohi[bin_]) == b + 1
        vlo, vhi = f32(tlo[bin_] - 0.5), f32(thi[bin_] - 0.5)                  # 512.0f * v, an f32 value
        assert f64(vlo) + 0.5 == tlo[bin_] and f64(vhi) + 0.5 == thi[bin_]
        ulp = f64(np.spacing(f32(b + 0.5)))
        assert 0 < (b + 0.5) - f64(vlo) <= ulp and 0 <= f64(vhi) - (b + 0.5) <= ulp, (k, vlo, vhi)
    # subnormals: squares that vanish, values that become inf and clip; squares that are subnormal themselves
    sub = rows["subnormal_all"]
    assert (np.abs(sub) < np.finfo(f32).tiny).all() and (sub != 0).sum() > 100 and not (sub * sub).any()
    o, c, _ = by["subnormal_all"]
    assert c and (sub == 0).sum() > 10 and not o.any()                        # its zeros became 0 * inf = NaN: the second length is NaN
    o, c, t = by["subnormal_dense"]
    sub = rows["subnormal_dense"]
    assert (sub != 0).all() and (np.abs(sub) < np.finfo(f32).tiny).all() and not (sub * sub).any()
    assert c and (o == int(512.0 / np.sqrt(128.0) + 0.5)).all()              # every entry inf, clipped to 0.2f: a flat row
    some = rows["subnormal_some"]
    assert ((some != 0) & (np.abs(some) < np.finfo(f32).tiny)).sum() > 20 and (some >= 1).sum() > 30
    tiny = rows["tiny_squares"]
    sq = tiny * tiny
    assert (sq > 0).all() and (sq < np.finfo(f32).tiny).all() and by["tiny_squares"][0].any()


def test_the_order_of_the_length_sum_matters():
    """the 32 group sums added last to first, or pairwise, give another length and another descriptor somewhere"""
    rows = Cs.norm_row_array()
    ref = M.sift_norm_f32(rows, 0.2)
    rev = M.sift_norm_f32(rows, 0.2, len_order=range(31, -1, -1))
    assert (rev != ref).any(), "no row of the case list tells the summation order"
    wide = dict(Cs.norm_rows())["wide_range"]
    sq = wide * wide
    g = ((sq[0::4] + sq[1::4]) + sq[2::4]) + sq[3::4]
    fwd, bwd = f32(0), f32(0)
    for i in range(32):
        fwd, bwd = fwd + g[i], bwd + g[31 - i]
    assert fwd != bwd
    # and the group sum itself: (sq0 + sq1) + (sq2 + sq3) is another number for some group of some row
    alt = (sq[0::4] + sq[1::4]) + (sq[2::4] + sq[3::4])
    allsq = rows * rows
    alt_all = (allsq[:, 0::4] + allsq[:, 1::4]) + (allsq[:, 2::4] + allsq[:, 3::4])
    g_all = ((allsq[:, 0::4] + allsq[:, 1::4]) + allsq[:, 2::4]) + allsq[:, 3::4]
    assert (alt != g).any() or (alt_all != g_all).any()


def test_the_pooling_order_matters():
    raw = Cs.model_raw()
    groups = [raw[i:i + 4] for i in range(0, len(raw) - 4, 4)]
    fwd = np.stack([M.pool(g) for g in groups])
    bwd = np.stack([M.pool(g, order=(3, 2, 1, 0)) for g in groups])
    assert (u32(fwd) != u32(bwd)).any(), "f32 pooling came out associative on every group"
    # pooling in f64 and rounding once is another histogram too
    wide = np.stack([g.astype(f64).sum(0).astype(f32) for g in groups])
    assert (u32(wide) != u32(fwd)).any()


@pytest.mark.parametrize("num_scales,start,end", Cs.NAMED_CONFIGS)
def test_mr_sizes(num_scales, start, end):
    """mrSize_k = mrSize * (startCoef + k * (endCoef - startCoef) / numScales) with the product before the division, in f64"""
    for mr in (1.0, 5.1962, 3.0 * 3.0 ** 0.5):
        got = M.mr_sizes(mr, num_scales, start, end)
        assert len(got) == num_scales + 1
        for k, g in enumerate(got):
            assert g == mr * (start + (k * (end - start)) / num_scales)
        assert got[0] == mr * start
    # the other bracketing is another number for some k of the sixteen scales: the formula is not a matter of taste
    if num_scales == 15:
        a = [5.1962 * (start + (k * (end - start)) / num_scales) for k in range(16)]
        b = [5.1962 * (start + k * ((end - start) / num_scales)) for k in range(16)]
        assert a != b


def test_dsp_regions_cross_the_direct_branch_boundary():
    from tests import describe_cases as DC
    regs = Cs.dsp_regions()
    assert 28 <= len(regs) <= 32
    for ns, a, b in Cs.CONFIGS[1:]:
        win = np.array([[DC.window_of(float(s), mr) for mr in M.mr_sizes(DC.MR_SIZE, ns, a, b)] for s in regs["det_kp"]["s"]])
        crossing = ((win == 0).any(1) & (win > 0).any(1)).sum()
        assert crossing >= 5 and (win == 0).all(1).sum() >= 3 and (win > 0).all(1).sum() >= 5, (ns, crossing)
    # the fast-extraction regions: direct at every scale, and the flag changes neither the window nor imageToPatchScale
    ns, a, b = Cs.FAST_CONFIG
    for mr in M.mr_sizes(DC.MR_SIZE, ns, a, b):
        x = float(mr) * Cs.FAST_S
        assert x == int(x) and DC.window_of(Cs.FAST_S, mr) == 0
        pis = 2 * int(x) + 1
        assert f32(f64(pis) / f64(41)) == f32(pis) / f32(41)
