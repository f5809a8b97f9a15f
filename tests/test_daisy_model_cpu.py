"""The DAISY model (tests/daisy_model.py) against the compiled reference's recorded results (tests/golden/daisy_ref.npz, written by
tools/make_daisy_fixture.py), the library's host tables against the model's and the fixture's, the claims of tests/daisy_cases.py,
and two experiments that show an ordering error cannot pass."""
import os

import numpy as np
import pytest

import daisy_cases as Cs
import daisy_model as M
import mods_amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "daisy_ref.npz")
DEFAULT, INI, ONE_RING, SMALL, TINY = Cs.PARAMS


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert [str(n) for n in g["names"]] == Cs.names(), "the fixture is not of this case list: rerun tools/make_daisy_fixture.py"
    assert tuple(tuple(int(v) for v in row) for row in g["params"]) == Cs.PARAMS
    return g


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_rows(got, ref, what):
    assert got.shape == ref.shape and not np.isnan(ref).any(), what
    bad = np.nonzero((u32(got) != u32(ref)).any(1))[0]
    assert len(bad) == 0, (what, [Cs.names()[i] for i in bad[:10]])


def row(name):
    return Cs.names().index(name)


def test_case_list():
    names = Cs.names()
    assert 15 <= len(names) <= 25 and len(set(names)) == len(names)
    p = Cs.patches()
    assert p.shape == (len(names), 41, 41) and p.dtype == np.float32 and np.isfinite(p).all()
    assert Cs.PARAMS == ((15, 3, 8, 8), (20, 3, 8, 8), (20, 1, 8, 8), (7, 2, 4, 8), (1, 3, 8, 8)) and Cs.NRMS == (0, 1, 2)
    for n in ("flat", "step_v", "textured_left", "half_even", "saturation", "border_only"):
        assert n in names


def test_model_equals_reference_bit_for_bit(golden):
    for s, P in enumerate(Cs.PARAMS):
        for nrm in Cs.NRMS:
            ref = golden["desc_%d_%d" % (s, nrm)]
            assert ref.shape == (len(Cs.names()), M.dim(P[1], P[2]))
            same_rows(Cs.model(P, nrm), ref, "%s, nrm_type %d" % (P, nrm))


def test_model_equals_the_recorded_intermediates(golden):
    assert [Cs.names()[i] for i in golden["planes_of"]] == list(Cs.PLANES_OF)
    assert Cs.names()[int(golden["cubes_of"])] == Cs.CUBES_OF and int(golden["cube_layer"]) == Cs.CUBE_LAYER
    k, layer = int(golden["cubes_of"]), int(golden["cube_layer"])
    for s, P in enumerate(Cs.PARAMS):
        info = Cs.info(P, M.NRM_FULL)
        for j, key in enumerate(("blurred", "dx", "dy")):
            assert np.array_equal(u32(info[key][golden["planes_of"]]), u32(golden["planes"][:, j])), key
        cubes = golden["cubes_%d" % s]
        # the reference's compute_histograms leaves row 40 and column 40 of a transposed cube unwritten; no sample reads them
        assert cubes.shape == (P[1], 40, 40) and cubes.any()
        assert np.array_equal(u32(info["cubes"][:, k, layer, :40, :40]), u32(cubes)), P


def test_tables(golden):
    assert np.array_equal(u32(M.gaussian_1d(5, 0.5)), u32(golden["k5"]))
    for s, P in enumerate(Cs.PARAMS + ((13, 3, 7, 8), (19, 2, 5, 8), (3, 1, 1, 8))):
        model, lib = M.tables(*P), mods_amd.daisy_tables(*P)
        for key in ("k5", "kos", "zin", "taps", "w"):
            assert np.array_equal(u32(model[key]), u32(lib[key])), (P, key)
        for key in ("fsz", "selected", "state", "base"):
            assert np.array_equal(model[key], lib[key]), (P, key)
        if P not in Cs.PARAMS:
            continue
        assert np.array_equal(u32(lib["taps"]), u32(golden["taps_%d" % s])), P
        assert np.array_equal(lib["selected"], golden["selected_%d" % s]), P
        assert np.array_equal(model["grid"], golden["grid_%d" % s]), P
        assert list(lib["selected"]) == list(range(P[1]))                     # ring r reads cube r at every case triple
    assert list(M.tables(*DEFAULT)["fsz"]) == [7, 13, 21, 27] and list(M.tables(*INI)["fsz"]) == [7, 17, 29, 37]
    assert list(M.tables(*ONE_RING)["fsz"]) == [7, 51] == [7, M.MAX_TAPS]         # sigma 10: the longest filter
    assert list(M.tables(*TINY)["fsz"]) == [7, 3, 3, 3]                           # the floor of filter_size
    for P in Cs.PARAMS:
        t = M.tables(*P)
        assert t["state"][0] == M.SAMPLED and t["base"][0] == 20 * 41 + 20 and list(t["w"][0]) == [1, 0, 0, 0]
        for f, n in enumerate(t["fsz"]):
            assert t["taps"][f, :n].min() > 0 and not t["taps"][f, n:].any()
            assert np.array_equal(t["taps"][f, :n], t["taps"][f, :n][::-1])          # symmetric, so only the order of adds matters


def test_zero_histograms_at_rad_20():
    """at the shipped ini's rad = 20 the +x and +y points of the outer ring give 8 zeros: histograms 17 and 19, exactly"""
    t = M.tables(*INI)
    assert [g for g in range(25) if t["state"][g] != M.SAMPLED] == [17, 19]
    assert list(t["state"][[17, 19]]) == [M.ZEROED, M.ZEROED]                 # 3 * (float)(20 / 3) is just below 20: int() gives 39
    assert [g for g in range(9) if M.tables(*ONE_RING)["state"][g] == M.SKIPPED] == [1, 3]          # 20 + 20 = 40: outside [0, 40)
    assert (M.tables(*DEFAULT)["state"] == M.SAMPLED).all()
    textured = [row(n) for n in Cs.names() if n.startswith(("random_", "levels_", "region_"))]
    zero = Cs.info(INI, M.NRM_PARTIAL)["zero_hist"][textured]
    assert [g for g in range(25) if zero[:, g].all()] == [17, 19] and not zero[:, [g for g in range(25) if g not in (17, 19)]].any()
    for nrm in Cs.NRMS:
        d = Cs.model(INI, nrm)[textured].reshape(len(textured), 25, 8)
        assert not d[:, [17, 19]].any() and d[:, 0].any(1).all()


def test_flat_patches_take_the_zero_norm_branches():
    for P in Cs.PARAMS:
        for name in ("flat", "zero"):
            k = row(name)
            assert Cs.info(P, M.NRM_PARTIAL)["zero_hist"][k].all() and Cs.info(P, M.NRM_FULL)["zero_norm"][k]
            assert Cs.info(P, M.NRM_SIFT)["rounds"][k] == 1 and not Cs.info(P, M.NRM_SIFT)["clips"][k].any()
            for nrm in Cs.NRMS:
                assert not Cs.model(P, nrm)[k].any()
        # (rad = 1 sees nothing of border_only either: test_border_only_reaches_inward_through_every_filter)
        others = [i for i, n in enumerate(Cs.names()) if n not in ("flat", "zero") and (n, P) != ("border_only", TINY)]
        assert not Cs.info(P, M.NRM_FULL)["zero_norm"][others].any()


def test_step_reaches_the_clip_and_a_second_round():
    k = row("step_v")
    for P, first in ((DEFAULT, 13), (INI, 13), (ONE_RING, 10), (SMALL, 16)):
        info = Cs.info(P, M.NRM_SIFT)
        assert info["rounds"][k] == M.MAX_ROUNDS and info["clips"][k][0] == first and (info["clips"][k][1:] > first).all(), P
        assert not np.array_equal(u32(Cs.model(P, M.NRM_SIFT)[k]), u32(Cs.model(P, M.NRM_FULL)[k]))
        assert Cs.model(P, M.NRM_SIFT)[k].max() == M.CLIP and Cs.model(P, M.NRM_FULL)[k].max() > M.CLIP
    # rad = 1: 25 alike histograms, nothing above the clip, one round, the same bits as NRM_FULL
    info = Cs.info(TINY, M.NRM_SIFT)
    assert info["rounds"][k] == 1 and not info["clips"][k].any()
    assert np.array_equal(u32(Cs.model(TINY, M.NRM_SIFT)[k]), u32(Cs.model(TINY, M.NRM_FULL)[k]))
    # both exits of the loop occur on textured patches too
    rounds = Cs.info(DEFAULT, M.NRM_SIFT)["rounds"]
    assert set(rounds.tolist()) == {1, M.MAX_ROUNDS} and rounds[row("random_0")] == 1 and rounds[row("region_1")] == M.MAX_ROUNDS


def test_textured_left_has_zero_histograms_beside_others():
    k = row("textured_left")
    for P, zero in ((DEFAULT, [1]), (INI, [1, 17, 19]), (ONE_RING, [1, 3]), (SMALL, [1])):
        z = Cs.info(P, M.NRM_PARTIAL)["zero_hist"][k]
        assert list(np.nonzero(z)[0]) == zero, P
        d = Cs.model(P, M.NRM_PARTIAL)[k].reshape(-1, 8)
        assert not d[z].any() and d[~z].any(1).all()
        norms = M.l2norm(d[~z])
        assert np.abs(norms - 1).max() < 1e-6


def test_half_even_and_saturation_pixels():
    p = Cs.patches()
    h = p[row("half_even")]
    fl = np.floor(h)
    half = h - fl == 0.5
    assert (half & (fl % 2 == 0)).sum() > 400 and (half & (fl % 2 == 1)).sum() > 400
    b = M.to_unit(h) / np.float32(1.0 / 255.0)
    got = np.rint(b)
    assert np.array_equal(got[half & (fl % 2 == 0)], fl[half & (fl % 2 == 0)])            # k + 0.5 -> k for even k
    assert np.array_equal(got[half & (fl % 2 == 1)], fl[half & (fl % 2 == 1)] + 1)        # k + 0.5 -> k + 1 for odd k
    s = p[row("saturation")]
    assert (s < 0).sum() > 200 and (s > 255).sum() > 200 and s.min() < -59 and s.max() > 330
    assert ((s < 0) & (s > -0.5)).any() and ((s > 255) & (s < 255.5)).any()
    u = M.to_unit(s)
    assert (u[s < 0] == 0).all() and (u[s > 255] == np.float32(255) * np.float32(1.0 / 255.0)).all() and u.min() == 0 and u.max() <= 1
    # rounding half up, or truncation, would change rows
    for wrong in (np.floor(h + 0.5), np.floor(h)):
        assert not np.array_equal(u32(M.describe(wrong[None])), u32(M.describe(h[None])))


def test_border_only_reaches_inward_through_every_filter():
    k = row("border_only")
    p = Cs.patches()[k]
    assert (p[2:39, 2:39] == 128).all() and len(np.unique(p[:2])) > 20
    for P in Cs.PARAMS[:4]:
        assert Cs.model(P, M.NRM_FULL)[k].any(), P
    # the centre of rad = 1 sees nothing of it: filters of 7 + 3 + 3 + 3 taps do not reach from the border to pixel 20
    assert not Cs.model(TINY, M.NRM_FULL)[k].any()


def test_the_order_of_operations_is_pinned():
    """columns before rows, or taps summed from the far end, give other bits on most cases at every parameter set"""
    pats = Cs.patches()
    for P in Cs.PARAMS:
        ref = Cs.model(P, M.NRM_FULL)
        for variant in ("swap", "reverse"):
            d = M.describe(pats, *P, nrm_type=M.NRM_FULL, variant=variant)
            differ = (u32(d) != u32(ref)).any(1)
            assert differ.sum() >= 10, (P, variant, int(differ.sum()))
            assert np.abs(d - ref).max() < 1e-3               # rows of unit norm: the same arithmetic, another rounding
