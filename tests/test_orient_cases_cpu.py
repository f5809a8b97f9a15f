"""CPU proof that the inputs of tests/orient_cases.py reach what they claim (the GPU comparisons are in tests/test_gpu_orient.py):
the identity harness hands the planted patches to interpolate() bit for bit, DetectOrientation on the composed image is
dominant_angles on the patches, every claim of a planted or geometric case holds in the model's report, and every mutation of
orient_model.MUTATIONS changes the answer of a named case."""
import numpy as np
import pytest

import orient_cases as cases
import orient_model as M
from common import same_records

F = np.float32


def _by_name():
    return {c["name"]: (i, c) for i, c in enumerate(cases.planted())}


@pytest.fixture(scope="module")
def composed(oracle):
    img, centres = cases.compose()
    return img, centres, cases.identity_regions(oracle.REGION, centres)


def test_families_and_names():
    P = cases.planted()
    assert len({c["name"] for c in P}) == len(P)
    assert cases.family_counts() == dict(ramps=2053, extremes=8, peaks=16, random=4 * cases.RANDOM_PER_KIND)
    assert all(np.isfinite(c["patch"]).all() for c in P)


def test_identity_harness_hands_over_the_planted_block(oracle, modsx, composed):
    img, centres, regs = composed
    P = cases.planted()
    assert cases.patch_scale(cases.MR_IDENTITY) == 1.0
    win = [(img.shape[1], img.shape[0], x, y, 1.0, 0.0, 0.0, 1.0, 41) for x, y in centres]
    box = [(img.shape[1], img.shape[0], x, y, 1.0, 0.0, 0.0, 1.0, int(cases.K_SIGMA * 1.0)) for x, y in centres]
    assert not modsx.check_borders(box).any() and not oracle.interpolate_check_borders(box).any()
    assert not modsx.check_borders(win).any() and not oracle.interpolate_check_borders(win).any()      # the truncation branch
    for k in range(len(P)):
        x, y = centres[k]
        got, outside = oracle.interpolate(img, x, y, 1.0, 0.0, 0.0, 1.0, 41, 41)
        assert not outside and np.array_equal(got, P[k]["patch"]), P[k]["name"]
        assert np.array_equal(img[y - 20:y + 21, x - 20:x + 21], P[k]["patch"])


@pytest.mark.parametrize("half,th,max_ang,upright", [(0, 0.8, 1, 0), (1, 0.8, 18, 0), (0, 1.0, 2, 1), (1, 1.0, 100, 0), (0, 0.8, 0, 1),
                                                     (0, 0.8, -1, 1)])
def test_detect_orientation_on_the_composed_image_is_dominant_angles_on_the_patches(oracle, composed, half, th, max_ang, upright):
    img, centres, regs = composed
    P = cases.planted()
    angles = [oracle.dominant_angles(c["patch"], half, th, max_ang) if max_ang > 0 else [] for c in P]
    want = cases.expected_records(regs, angles, max_ang, upright)
    got = oracle.detect_orientation(img, regs, mr_size=cases.MR_IDENTITY, half=half, max_ang=max_ang, th=th, upright=upright)
    assert len(got) == len(want) == sum(len(a) for a in angles) + upright * len(P)
    assert same_records(got, want)
    if max_ang > 0 and not upright:
        assert np.array_equal(cases.counts_per_centre(got, centres), [len(a) for a in angles])


# ---- reach -------------------------------------------------------------------------------------------------------------------------
def test_every_bin_table_entry_is_hit(oracle):
    A = cases.analysis(oracle)
    v = A["bin"] >= 0
    entries = set(np.unique((A["code"] * 256 + A["idx"])[v & ~A["special"]]).tolist())
    assert entries == set(range(2048))
    assert (v & A["special"]).any()
    # the ramps alone do it, each with the entry it claims
    for i, c in enumerate(cases.planted()):
        if c["family"] != "ramps":
            continue
        vi = v[i]
        if "entry" in c["claim"]:
            code, idx = c["claim"]["entry"]
            hit = vi & (A["code"][i] == code) & (A["idx"][i] == idx) & ~A["special"][i]
            assert hit.any(), c["name"]
            if c["claim"].get("one_bin"):
                assert hit.sum() == vi.sum() == M.NVOTERS, c["name"]
        if c["claim"].get("special"):
            assert (A["special"][i] & vi).sum() == M.NVOTERS, c["name"]
    # idx 255 with |x| > |y|: the quotient rounds up to 255.0 (the only way to the upper clamp of the index)
    bx, by = cases.BIG_IDX255
    assert bx > by and (F(255) * by) / bx == F(255)


def test_vote_count_claims(oracle):
    A = cases.analysis(oracle)
    r, c = M.voting_list()
    seen = set()
    for i, case in enumerate(cases.planted()):
        cl, votes = case["claim"], A["votes"][i]
        if cl.get("one_bin"):
            assert votes.max() == votes.sum() > 0, case["name"]
            if "lane" not in cl:
                assert votes.max() == 1245, case["name"]
        if "bin" in cl:
            assert votes[cl["bin"]] == votes.sum() == 1245, case["name"]
        if "nvotes" in cl:
            assert votes.sum() == cl["nvotes"], case["name"]
        if "mag" in cl:
            assert (A["mag"][i][1:-1, 1:-1] == cl["mag"]).all(), case["name"]
        if "counts" in cl:
            assert {int(b): int(votes[b]) for b in np.nonzero(votes)[0]} == cl["counts"], case["name"]
            seen |= set(cl["counts"].values()) | {0}
        if "lane" in cl:
            pos = np.nonzero(A["bin"][i][r, c] >= 0)[0]          # positions in the voting list
            assert len(pos) == 21 and (pos // 21 == cl["lane"]).all() and (pos % 21 == np.arange(21)).all(), case["name"]
    assert {0, 1, 7, 8, 9} <= seen
    by = _by_name()
    assert A["votes"][by["ramp/angle_pi"][0]][36] == 1245                  # everything in the slot nothing reads
    assert A["votes"][by["ramp/c3_i000"][0]][36] == 1245
    assert A["votes"][by["ramp/angle_minus_pi"][0]][0] == 1245 and A["votes"][by["ramp/angle_minus_pi_y0"][0]][0] == 1245
    assert len(cases.single_row_lanes()) >= 3
    # the random patches spread their votes; the low-contrast ones have gradients on both sides of 1
    for i, case in enumerate(cases.planted()):
        if case["name"].startswith("random/lowcontrast"):
            m = A["mag"][i][1:-1, 1:-1]
            assert (m > 1).any() and (m <= 1).any(), case["name"]


def test_peak_claims(oracle):
    A = cases.analysis(oracle)
    P = cases.planted()
    reports = {}
    for half in (0, 1):
        for th in (0.8, 1.0):
            reports[(half, th)] = M.dominant_angles_batch(oracle, None, half, th, -1, analysis=A)[1]
    plain = reports[(0, 0.8)]
    counts_seen = set()
    for i, case in enumerate(P):
        cl = case["claim"]
        for key, n in cl.get("npeaks", {}).items():
            assert reports[key]["peak"][i].sum() == n, (case["name"], key)
            if key == (0, 0.8):
                counts_seen.add(n)
        if "peak_bins" in cl:
            assert list(np.nonzero(plain["peak"][i])[0]) == cl["peak_bins"], case["name"]
        if cl.get("equal_weights"):
            w = A["raw"][i][[0, 27]]
            assert w[0] == w[1] > 0 and A["raw"][i][18] == w[0] + w[0], case["name"]
        if "tie" in cl:
            a, b = cl["tie"]
            s = reports[(0, 1.0)]
            assert s["smoothed"][i][a] == s["smoothed"][i][b] == s["smoothed"][i].max() == s["thresh"][i], case["name"]
        if "plateau" in cl:
            a, b = cl["plateau"]
            assert plain["smoothed"][i][a] == plain["smoothed"][i][b] == plain["smoothed"][i].max(), case["name"]
        if "fold_tie" in cl:
            a, b = cl["fold_tie"]
            f = reports[(1, 0.8)]
            assert f["folded"][i][a] == f["folded"][i][b] == f["folded"][i].max() and not f["peak"][i][[a, b]].any(), case["name"]
            assert plain["smoothed"][i][a] != plain["smoothed"][i][b]
        if cl.get("rising"):
            v = plain["folded"][i][np.nonzero(plain["peak"][i])[0]]
            assert (np.diff(v) > 0).all(), case["name"]
    assert {0, 1, 2, 3, 4, 5, 18} <= counts_seen
    npk = plain["peak"].sum(1)
    assert npk.max() == cases.MAX_PEAKS == 18            # strict peaks are never adjacent: 18 is all a 36-bin histogram can have
    for max_angles in (1, 2, cases.MAX_PEAKS - 1):       # a case with more peaks than every cut that can bind
        assert (npk > max_angles).any()
    # plain and Half peaks differ somewhere, and the fold changes the count of the case that claims it
    assert (reports[(0, 0.8)]["peak"] != reports[(1, 0.8)]["peak"]).any()


# ---- geometric cases ------------------------------------------------------------------------------------------------------------
def _classify(oracle, modsx, reg, mr, rows, cols):
    box, win = cases.border_tuples(reg, mr, rows, cols)
    fails = bool(modsx.check_borders([box])[0])
    touch = bool(modsx.check_borders([win])[0])
    assert fails == bool(oracle.interpolate_check_borders([box])[0]) and touch == bool(oracle.interpolate_check_borders([win])[0])
    outside = cases.taps_outside(reg, mr, rows, cols)
    if fails:
        return "dropped", outside
    return ("inside" if not touch else "touch_inside" if outside == 0 else "overhang"), outside


def test_geometric_claims(oracle, modsx):
    seen = {}
    for group, img in ((cases.GEOMETRIC, cases.textured_image()), (cases.SMALL_GEOMETRIC, cases.small_image())):
        rows, cols = img.shape
        for name, reg, claims in group:
            for mr in cases.MR_SIZES:
                cls, outside = _classify(oracle, modsx, reg, mr, rows, cols)
                if mr in claims:
                    assert cls == claims[mr], (name, mr, cls, outside)
                if cls == "inside":
                    assert outside == 0, (name, mr)
                if cls == "overhang":
                    assert outside > 0
                seen.setdefault((cls, mr), []).append((name, outside))
                # the oracle's interpolate() agrees about the taps it zeroes
                if cls != "dropped":
                    x, y, s, a11, a12, a21, a22 = reg
                    sc = F(cases.patch_scale(mr) * s)
                    _, zeroed = oracle.interpolate(img, x, y, *(float(F(F(v) * sc)) for v in (a11, a12, a21, a22)), 41, 41)
                    assert zeroed == (outside > 0), (name, mr)
    for mr in cases.MR_SIZES:
        assert ("inside", mr) in seen and ("dropped", mr) in seen
    assert ("touch_inside", 5.1962) in seen and ("touch_inside", 20.0) in seen and ("touch_inside", 8.0) in seen
    assert len(seen[("overhang", 20.0)]) >= 8 and len(seen[("overhang", 8.0)]) >= 5
    # over each edge and a corner, counted from the restated coordinates
    img = cases.textured_image()
    rows, cols = img.shape
    by = {c[0]: c[1] for c in cases.GEOMETRIC}
    for name, test in (("over_left", lambda X, Y: X < 0), ("over_right", lambda X, Y: np.floor(X) >= cols - 1),
                       ("over_top", lambda X, Y: Y < 0), ("over_bottom", lambda X, Y: np.floor(Y) >= rows - 1),
                       ("over_corner", lambda X, Y: (X < 0) & (Y < 0))):
        WX, WY = cases.tap_coordinates(by[name], 20.0)
        assert test(WX, WY).sum() > 100, name
    assert img.min() < -20 and img.max() > 50 and (img < 0).mean() > 0.2
    # the near-zero shape: every tap in one pixel
    WX, WY = cases.tap_coordinates(by["nearzero"], 20.0)
    assert len(np.unique(np.floor(WX))) == 1 and len(np.unique(np.floor(WY))) == 1
    assert by["negdet_s2"][3] * by["negdet_s2"][6] - by["negdet_s2"][4] * by["negdet_s2"][5] < 0
    assert any(r[0] != int(r[0]) or r[1] != int(r[1]) for r in by.values())
    s = cases.small_image()
    assert s.shape == (30, 30) and min(s.shape) < 41


def test_tap_coordinates_restated_like_the_oracle(oracle):
    """a ramp image makes interpolate() return its own sample coordinates: I = x and I = y, inside the image"""
    rows, cols = 200, 260
    yy, xx = np.mgrid[0:rows, 0:cols].astype(F)
    reg = dict((c[0], c[1]) for c in cases.GEOMETRIC)["shear_s2"]
    WX, WY = cases.tap_coordinates(reg, 5.1962)
    x, y, s, a11, a12, a21, a22 = reg
    sc = F(cases.patch_scale(5.1962) * s)
    args = [float(F(F(v) * sc)) for v in (a11, a12, a21, a22)]
    gx, _ = oracle.interpolate(xx, x, y, *args, 41, 41)
    gy, _ = oracle.interpolate(yy, x, y, *args, 41, 41)
    assert np.abs(gx - WX).max() < 1e-3 and np.abs(gy - WY).max() < 1e-3


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
# mutation -> (the case that notices it, half, th, max_angles)
NOTICED_BY = {
    "peak_ge": ("peaks/plateau_two_bins", 0, 0.8, -1),
    "thresh_gt": ("peaks/tie_two_maxima", 0, 1.0, -1),
    "mag_ge": ("extreme/mag_exactly_1", 0, 0.8, -1),
    "reverse_raster": ("random/white_00", 0, 0.8, -1),
    "smooth_right_first": ("random/white_00", 0, 0.8, -1),
    "five_passes": ("peaks/npeaks_5", 0, 0.8, -1),
    "bin36_to_0": ("ramp/angle_pi", 0, 0.8, -1),
    "bin36_to_35": ("ramp/angle_pi", 0, 0.8, -1),
    "cut_largest": ("peaks/rising_three", 0, 0.8, 1),
}


@pytest.mark.parametrize("mutation", sorted(NOTICED_BY))
def test_mutation_changes_a_named_case(oracle, mutation):
    name, half, th, max_angles = NOTICED_BY[mutation]
    i, case = _by_name()[name]
    good, _ = M.dominant_angles(oracle, case["patch"], half, th, max_angles)
    bad, _ = M.dominant_angles(oracle, case["patch"], half, th, max_angles, mut=(mutation,))
    assert np.array_equal(good.view(np.int32), oracle.dominant_angles(case["patch"], half, th, max_angles).view(np.int32))
    assert not (len(good) == len(bad) and np.array_equal(good.view(np.int32), bad.view(np.int32))), (mutation, name)


def test_floor_for_truncation_cannot_be_noticed(oracle):
    """MUTATIONS lists "bin_floor"; no finite patch can tell floor from truncation in (int)(36 * (ori / pi + 1) / 2): atan2LUTff
    returns one of 2049 angles, all >= -pi, so the expression is never negative.  Proven here over every angle instead of by a
    case; the smallest value is exactly 0 (angle -pi)."""
    assert set(M.MUTATIONS) == set(NOTICED_BY) | {"bin_floor"}
    code, idx = np.divmod(np.arange(2048), 256)
    ang = np.concatenate([M.angle_of_case(oracle.atan_lut(), code, idx), [F(0)]]).astype(F)
    v = (F(36) * (ang / F(np.pi) + F(1.0))) / F(2.0)
    assert v.min() == 0 and np.array_equal(np.floor(v), np.trunc(v))
    assert np.array_equal(M.bin_of_angle(ang), M.bin_of_angle(ang, floor=True))
