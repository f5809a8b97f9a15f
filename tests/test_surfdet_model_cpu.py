"""CPU: tests/surfdet_model.py, the numpy restatement of OpenSURF's FastHessian that the GPU tests compare the library with, equals
the compiled reference bit for bit on every case of tests/surfdet_cases.py (tests/golden/surfdet_ref.npz, recorded by
tools/make_surfdet_fixture.py), and the cases reach what they claim.

The width quotient.  getResponse reads a denser layer at scale = this->width / src->width, an integer division the model and the
kernels restate.  For the layer pairs getIpoints forms (the denser layer has k = 1, 2 or 4 times the nominal density of t) the
quotient is k + rem / t->width with rem <= k - 1 <= 3, so it leaves the nominal ratio only where t is at most 3 wide -- and
isExtremum's bounds test (border >= 1) passes no position of such a layer.  A quotient of 17, or any other than the nominal one, is
therefore never READ: test_width_quotient_is_nominal_wherever_a_position_passes_the_bounds_test shows it for every width, and the
239- and 478-wide five-octave cases are kept as plane and extremum parity with the quotients they use listed.  No case can change
under a nominal ratio, so no such test exists here."""
import os

import numpy as np
import pytest

import surfdet_cases as SC
import surfdet_model as M
from conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "surfdet_ref.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIXTURE)
    assert list(z["names"]) == SC.names(), "the fixture was recorded for another case list: rerun tools/make_surfdet_fixture.py"
    return z


def _planes(m):
    return [m["integral"]] + m["resp"]


@pytest.mark.parametrize("k,name", list(enumerate(SC.names())))
def test_model_equals_the_compiled_reference(fx, k, name):
    m = SC.model(name)
    g = lambda key: fx["c%02d_%s" % (k, key)]                       # noqa: E731
    assert np.array_equal(np.array(m["layers"], np.int32), g("layers"))
    assert np.array_equal(np.stack([M.digest(a) for a in _planes(m)]), g("digests")), "integral image / response planes"
    assert np.array_equal(np.stack([M.digest(a) for a in m["lap"]]), g("lap_digests")), "laplacian planes"
    got = np.stack([a.reshape(-1)[M.sample_index(a.size)] for a in _planes(m)])
    assert got.tobytes() == g("samples").tobytes()
    assert np.array_equal(m["extrema"], g("extrema")), "extremum list and its order"
    assert m["points"].dtype == np.float32 and m["points"].tobytes() == g("points").tobytes(), "points and their order"
    assert np.array_equal(m["points_lap"], g("points_lap"))
    if name in SC.WHOLE_PLANES:
        assert m["integral"].tobytes() == g("integral").tobytes()
        for j in range(len(m["layers"])):
            assert m["resp"][j].tobytes() == g("resp_%d" % j).tobytes() and np.array_equal(m["lap"][j], g("lap_%d" % j)), j


def test_fixture_is_small():
    assert os.path.getsize(FIXTURE) < 256 * 1024


def test_integral_is_the_serial_loop():
    """np.cumsum in f32 is one add after the other: the loops of Integral() on a case image give the same bits"""
    img = SC.case("s31x33_is1")[1]
    g = img * np.float32(1.0 / 255.0) + np.float32(0.0)
    want = np.zeros_like(g)
    for i in range(g.shape[0]):
        rs = np.float32(0.0)
        for j in range(g.shape[1]):
            rs = np.float32(rs + g[i, j])
            want[i, j] = rs + want[i - 1, j] if i else rs
    assert M.integral(img).tobytes() == want.tobytes()


def test_parameter_normalisation():
    t = np.float32(0.0004)
    assert M.normalise(4, 4, 2, 0.0004) == (4, 4, 2, t)
    assert M.normalise(0, 0, 0, -1.0) == (5, 4, 2, t) and M.normalise(5, 5, 7, -0.0) == (5, 4, 2, np.float32(0))
    assert M.normalise(1, 1, 1, 0.0) == (1, 1, 1, np.float32(0)) and M.normalise(-3, 9, 6, 2.5) == (5, 4, 6, np.float32(2.5))
    assert [L[3] for L in M.geometry(480, 478, octaves=0, init_sample=2)] == list(M.FILTERS)
    assert [L[:3] for L in M.geometry(480, 478, octaves=0, init_sample=2)][-1] == (14, 15, 32)
    with pytest.raises(ValueError):
        M.geometry(12, 40, **M.INI)            # 12 / 2 / 8 == 0
    # the cases that ask for a default get it
    assert SC.model("s320x240_o0")["params"][0] == 5 and len(SC.model("s320x240_o0")["layers"]) == 12
    assert SC.model("s320x240_tneg")["params"][3] == t and SC.model("s320x240_iv9")["params"][1] == 4
    for a, b in (("s320x240_tneg", "s320x240"), ("s320x240_iv9", "s320x240")):
        assert SC.model(a)["points"].tobytes() == SC.model(b)["points"].tobytes()


# ---------------------------------------------------------------------------------------------- the cases reach what they claim
def _octaves_with_points():
    seen = set()
    for name in SC.names():
        m = SC.model(name)
        seen |= set(m["extrema"][m["accepted"]][:, 0].tolist())
    return seen


def test_every_octave_has_an_accepted_point():
    assert _octaves_with_points() == {0, 1, 2, 3, 4}
    m = SC.model("s400x400_is1_o5")
    assert 4 in set(m["extrema"][m["accepted"]][:, 0].tolist()), "the fifth octave's point comes from the 400 x 400 case"


def test_each_of_the_three_offset_tests_rejects_an_extremum():
    rej = np.zeros(3, int)
    for name in SC.names():
        x = SC.model(name)["x"]
        rej += [(np.abs(x[:, j]) >= 0.5).sum() for j in (2, 1, 0)]          # xi, xr, xc
        m = SC.model(name)
        assert np.array_equal(m["accepted"], (np.abs(x) < 0.5).all(axis=1))
    assert (rej > 0).all(), rej
    # ... and each alone: an extremum that only this test rejects
    alone = np.zeros(3, int)
    for name in SC.names():
        bad = np.abs(SC.model(name)["x"]) >= 0.5
        for j in range(3):
            alone[j] += int((bad[:, j] & (bad.sum(axis=1) == 1)).sum())
    assert (alone > 0).all(), alone


def test_box_clamps_and_the_max_act():
    for name in ("borders_320x240", "borders_129x48_is1", "s30x30_is1"):
        st = SC.model(name)["stats"]
        assert min(st["top"], st["left"], st["bottom"], st["right"]) > 0, (name, st)
    assert SC.model("borders_129x48_is1")["stats"]["max0"] > 0 and SC.model("s320x240")["stats"]["max0"] > 0
    # a point found where the boxes were clamped: within the filter's reach of a border
    m = SC.model("borders_320x240")
    assert len(m["points"]) > 0


def test_smallest_sizes_and_the_flat_image():
    assert len(SC.model("s31x33_is1")["points"]) >= 1
    assert len(SC.model("s30x30_is1")["extrema"]) == 0            # 30 x 30 leaves 6 x 6 candidates; this seed has no maximum there
    assert len(SC.model("flat_320x240")["extrema"]) == 0 and (np.concatenate([r.reshape(-1) for r in SC.model("flat_320x240")["resp"]]) == 0).mean() > 0.5
    m = SC.model("dots320x240_is1_t0")
    assert len(m["extrema"]) > 600 and len(m["points"]) > 500, "thresh = 0: enough points to outgrow a fresh point buffer"
    for w in (63, 64, 65, 129):
        assert len(SC.model("s%dx48" % w)["points"]) >= 1


def test_tree_order_row_sum_changes_named_digests():
    for name in ("s65x48", "s320x240"):
        _, img, par = SC.case(name)
        a, b = M.integral(img), M.integral(img, row_sum="tree")
        assert a.tobytes() != b.tobytes() and np.allclose(a, b, rtol=1e-5)
        assert not np.array_equal(M.digest(a), M.digest(b))
    _, img, par = SC.case("s65x48")
    t = M.detect(img, row_sum="tree", **par)
    m = SC.model("s65x48")
    assert any(x.tobytes() != y.tobytes() for x, y in zip(t["resp"], m["resp"])), "the response digests change with it"


def test_width_quotient_is_nominal_wherever_a_position_passes_the_bounds_test():
    """every layer pair of getIpoints, every layer-0 width 1 .. 20000 and init_sample 1 .. 6: where the t layer is wide enough for
    the bounds test to pass a column (c > border and c < width - border with border >= 1: width >= 4) the width quotient is the
    nominal step ratio; where it differs the t layer has at most 3 columns"""
    w0 = np.arange(1, 20001)
    seen_other = 0
    for o in range(5):
        for i in (0, 1):
            ib, im, it = M.FILTER_MAP[o][i:i + 3]
            dens = lambda k: 0 if k < 4 else (k - 2) // 2            # noqa: E731  -- the octave (halvings) of layer k
            tw = w0 >> dens(it)
            for src in (ib, im):
                sw, nominal = w0 >> dens(src), 1 << (dens(it) - dens(src))
                ok = tw > 0
                q = sw[ok] // tw[ok]
                other = q != nominal
                seen_other += int(other.sum())
                assert (tw[ok][other] <= 3).all()
                border_min = 1
                assert (tw[ok][other] - border_min <= border_min + 1).all()       # no c with border < c < width - border
    assert seen_other > 0, "the quotient does leave the nominal ratio somewhere (on layers no position of which is tested)"
    # the five-octave cases of width quotient fame: the quotients their scans used, all nominal; the model with the nominal ratio
    # in place of the division is the same function on them
    for name in ("s239x300_is1_o5", "s478x480_is2_o5", "s400x400_is1_o5"):
        m = SC.model(name)
        assert len(m["layers"]) == 12 and m["layers"][-1][0] == (14 if name != "s400x400_is1_o5" else 25)
        assert {q for _, _, q in m["quotients"]} <= {1, 2, 4}
        _, img, par = SC.case(name)
        n = M.detect(img, nominal_quotient=True, **par)
        assert n["points"].tobytes() == m["points"].tobytes() and np.array_equal(n["extrema"], m["extrema"])
