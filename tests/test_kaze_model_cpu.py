"""CPU: tests/kaze_model.py -- the numpy restatement of the KAZE detector that the GPU tests compare the library with -- equals
tests/golden/kaze_ref.npz, what the reference's AKAZE sources compute when compiled unmodified against tools/kaze_standin/
(tools/make_kaze_fixture.py), at every recorded stage and list; the model's blur is held to the oracle's; the case list is proven to
reach what tests/kaze_cases.py claims; and two deliberate mistakes each change a named case.

The upper-level rejection of Find_Scale_Space_Extrema (AKAZE.cpp:363-384) is unreachable, and test_the_upper_level_pass_rejects_
nothing says why; the planted case scan_b holds the nearest thing, which the first pass settles."""
import os

import numpy as np
import pytest

import kaze_cases as KC
import kaze_model as M
from conftest import ROOT

PLANES = ("Lt", "Lsmooth", "Lflow", "Ldet")
LISTS = ("raw", "rawv", "aux", "upper", "final")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "kaze_ref.npz"))


def same_lists(m, fx, pre, what):
    for key in LISTS:
        g, w = np.ascontiguousarray(m[key]), fx[pre + key]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, key)


def test_the_fixture_lists_the_cases(fixture):
    assert list(fixture["names"]) == KC.names() and list(fixture["planted"]) == sorted(KC.PLANTED)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kaze_ref.npz")) < 1000000


@pytest.mark.parametrize("name", KC.names())
def test_model_equals_the_compiled_reference_at_every_stage(fixture, name):
    k = KC.names().index(name)
    pre = "c%02d_" % k
    m = KC.model(name)
    lv, ref = m["levels"], fixture[pre + "levels"]
    assert len(lv) == len(ref) and m["omax"] == int(fixture[pre + "omax"])
    for i, L in enumerate(lv):
        assert (L["octave"], L["sublevel"], L["rows"], L["cols"], L["sigma_size"], len(L["tau"])) == tuple(int(v) for v in ref[i]), i
        assert L["esigma"] == fixture[pre + "sigmas"][i, 0] and L["etime"] == fixture[pre + "sigmas"][i, 1], i
        assert L["tau"].tobytes() == fixture[pre + "tau"][i, :len(L["tau"])].tobytes(), i
    assert m["kcontrast"] == fixture[pre + "kcontrast"] and m["hmax"] == fixture[pre + "hmax"]
    assert np.array_equal(m["hist"], fixture[pre + "hist"])
    flat = [(nm, i, a) for nm in PLANES for i, a in enumerate(m[nm])]
    assert len(flat) == len(fixture[pre + "digests"])
    for j, (nm, i, a) in enumerate(flat):
        want = fixture[pre + "samples"][j]
        got = a.reshape(-1)[M.sample_index(a.size)]
        assert M.same(got, want), (nm, i, "samples")
        assert np.array_equal(M.digest(a), fixture[pre + "digests"][j]), (nm, i, "digest")
        if name in KC.WHOLE_PLANES:
            assert M.same(a, fixture[pre + "%s_%d" % (nm, i)]), (nm, i)
    same_lists(m, fixture, pre, name)


@pytest.mark.parametrize("name", sorted(KC.PLANTED))
def test_model_equals_the_compiled_reference_on_the_planted_planes(fixture, name):
    same_lists(KC.model(name), fixture, "p_%s_" % name, name)


def test_blur_is_the_oracles(oracle):
    """the model's two-pass Gaussian in the oracle's border mode is oracle.gaussian_blur_xy bit for bit, at AKAZE's two kernel sizes
    (9 taps: the long row pass; 5 taps: the short symmetric one); the library's border mode differs in the border pixels only"""
    assert (M.blur_ksize(1.6), M.blur_ksize(1.0)) == (9, 5)
    for w, h in ((61, 50), (128, 96)):
        img = np.asarray(KC.blobs(w, h), np.float32) * np.float32(1.0 / 255.0)
        for sigma in (1.6, 1.0):
            n, s = M.blur_ksize(sigma), float(np.float32(sigma))
            assert M.gaussian_kernel(n, s).tobytes() == oracle.gaussian_kernel(n, s).tobytes()
            ref = oracle.gaussian_blur_xy(img, n, n, s, s)
            assert M.blur(img, n, s, border="reflect").tobytes() == ref.tobytes()
            r = n // 2
            rep = M.blur(img, n, s)
            assert rep[r:-r, r:-r].tobytes() == ref[r:-r, r:-r].tobytes() and rep.tobytes() != ref.tobytes()


def test_the_cases_reach_what_they_claim():
    st = {n: KC.model(n)["stats"] for n in KC.names()}
    md = {n: KC.model(n) for n in KC.names()}
    # 1, 2, 3 and 4 surviving octaves, and the 80 x 40 cut on each side
    for name, octaves in KC.OCTAVES.items():
        assert md[name]["omax"] == octaves and len(md[name]["levels"]) == 4 * octaves, name
    for name, (w, h) in (("s159x96", (79, 48)), ("s160x96", (80, 48)), ("s176x79", (88, 39)), ("s176x80", (88, 40))):
        img = KC.case(name)[1]
        assert (img.shape[1] // 2, img.shape[0] // 2) == (w, h) and (md[name]["omax"] == 2) == (w >= 80 and h >= 40), name
    # both resize paths: the general table on both axes, and with one axis exact
    assert st["s177x145"]["resize"] == ["area"] and st["s176x145"]["resize"] == ["area"] and st["s176x144"]["resize"] == ["exact"]
    assert KC.case("s176x145")[1].shape == (145, 176)
    assert all(len(e) == 2 and e[0][1] == e[1][1] == 0.5 for e in M.area_table(176, 88))
    assert any(len(e) == 3 for e in M.area_table(145, 72)) and any(len(e) == 3 for e in M.area_table(177, 88))
    # every image case with more than one octave diffuses over all its levels; the four-octave one takes the 166 steps
    assert sum(len(L["tau"]) for L in md["s640x320"]["levels"]) == 166
    # a level with maxima, none inside the smax margin
    s = st["s160x96"]
    assert any(s["maxima"][i] > 0 and s["inside"][i] == 0 for i in range(4, 8)), s
    # the flat image: k = 0, NaN planes, no maximum
    f = md["flat_128x96"]
    assert f["kcontrast"] == 0 and f["hmax"] == 0 and not f["hist"].any() and len(f["raw"]) == 0 and len(f["final"]) == 0
    assert np.isnan(f["Lflow"][1]).all() and np.isnan(f["Lt"][1][1:-1]).all() and np.isfinite(f["Lt"][1][0, 0]) and np.isnan(f["Ldet"][2]).any()
    # the histogram walk that ends below its threshold
    assert st["s176x144_p12"]["k_branch"] == "0.03" and md["s176x144_p12"]["kcontrast"] == np.float32(0.03)
    assert all(st[n]["k_branch"] == "walk" for n in KC.names() if n != "s176x144_p12")
    # the M-SURF margin drops points the default keeps
    assert len(md["s176x144_msurf"]["final"]) < len(md["s176x144"]["final"])
    assert np.array_equal(md["s176x144_msurf"]["raw"], md["s176x144"]["raw"])
    # real images have keypoints, and their first pass sees both outcomes of the lower-level comparison
    assert len(md["s640x320"]["final"]) > 100 and st["s640x320"]["lower_keep"] > 0 and st["s640x320"]["lower_drop"] > 0


def test_the_planted_cases_reach_what_they_claim():
    a, b = KC.model("scan_a")["stats"], KC.model("scan_b")["stats"]
    assert a["same_keep"] >= 1 and a["same_drop"] >= 1 and a["lower_keep"] >= 2 and a["lower_drop"] >= 1 and a["replaced"] >= 3, a
    assert a["out_left"] == a["out_right"] == a["out_top"] == a["out_bottom"] == 1, a
    assert a["erased"] == 1 and a["singular_after"] == 1 and a["singular_first"] == 0, a
    assert b["singular_first"] == 1 and b["erased"] == 0, b
    # a lower level of the octave below was compared: a point of level 4 sits in the entry a point of level 3 opened
    fa = KC.model("scan_a")
    assert any(p["class_id"] == 4 and p["x"] == 200 and p["y"] == 100 for p in fa["aux"])
    # the singular point after a solved one takes the previous point's offsets: the two share their fractional parts
    fin = fa["final"]
    k = [i for i, p in enumerate(fin) if abs(p["x"] - 120) < 1 and abs(p["y"] - 200) < 1 and p["class_id"] == 0]
    assert len(k) == 1 and k[0] > 0
    prev = fin[k[0] - 1]
    assert fin[k[0]]["x"] - 120 == prev["x"] - 90 and fin[k[0]]["y"] - 200 == prev["y"] - 200 and prev["x"] != 90
    # the singular point that comes first stays where it is
    fb = KC.model("scan_b")["final"]
    assert fb[0]["x"] == 60 and fb[0]["y"] == 60


def test_the_upper_level_pass_rejects_nothing():
    """The second pass of Find_Scale_Space_Extrema drops a point P of level i when a LATER entry Q of level i + 1 lies within P.size
    and is stronger.  No list the first pass leaves can hold such a pair.  Q is of a higher level, so it is scanned after P and meets P
    in the first pass, which tests the same distance against the larger Q.size over entries of level i and i + 1 in list order and
    stops at the first one in reach.  If that is P, Q replaces P or is dropped.  If it is an earlier entry E, a stronger Q takes E's
    place, which lies BEFORE P, where the second pass (j > i) does not look, and a weaker Q is dropped.  So the rejection cannot
    fire; every case, planted or not, confirms it, and scan_b plants the nearest thing: Q one pixel from P, one level up, stronger."""
    for name in KC.names() + sorted(KC.PLANTED):
        m = KC.model(name)
        assert m["stats"]["upper_rejected"] == 0 and m["aux"].tobytes() == m["upper"].tobytes(), name
    b = KC.model("scan_b")
    assert b["stats"]["lower_keep"] == 1 and any(p["class_id"] == 1 and p["x"] == 101 and p["y"] == 70 for p in b["upper"])
    assert not any(p["class_id"] == 0 and p["x"] == 100 and p["y"] == 70 for p in b["upper"])


def test_another_tap_order_changes_a_named_case():
    """taps in descending index order: same products, another order of the f32 adds"""
    _, img, par = KC.case("t61x50")
    good, bad = KC.model("t61x50"), M.detect(img, tap_order="descending", **par)
    assert not M.same(bad["Ldet"][0], good["Ldet"][0])
    assert not M.same(bad["Lflow"][1], good["Lflow"][1])


def test_an_unpermuted_tau_list_changes_a_named_case(fixture):
    """fed_tau_by_process_time without reordering: the same steps in ascending order"""
    _, img, par = KC.case("t61x50")
    good, bad = KC.model("t61x50"), M.detect(img, reordering=False, **par)
    k = KC.names().index("t61x50")
    for i in range(1, 4):
        t = bad["levels"][i]["tau"]
        assert sorted(t) == sorted(good["levels"][i]["tau"]) and list(t) == sorted(t)
    # three steps permute onto themselves (kappa 1, modulus 5); the four steps of level 3 do not (kappa 2: 1, 3, 0, 2)
    t = bad["levels"][3]["tau"]
    assert len(t) == 4 and t.tobytes() != fixture["c%02d_tau" % k][3, :4].tobytes()
    assert M.same(bad["Lt"][2], good["Lt"][2]) and not M.same(bad["Lt"][3], good["Lt"][3])
