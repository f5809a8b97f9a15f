"""CPU: the inputs of the pyramid parity suite (tests/pyramid_cases.py) reach what tests/test_gpu_pyramid.py relies on.
That module compares the scale-space kernels with the oracle plane by plane and extremum by extremum; this one proves, from
the oracle (orc_scan_levels' report, blur_ksize) and the library's host-only tile rule (mods_amd.blur_geometry) alone, that
the comparisons run where the kernels can go wrong.  Every condition is a condition on the REFERENCE.

  - Blur: one sigma per instantiated half width R = 1 .. 8 (ksize 3 .. 17) and one that must be refused (ksize 19); the small
    shapes lie on both sides of the 64-column and 16-row tile edges and all take 16-row tiles.
  - Tile height: 16353 x 257 is exactly 2560 32-row tiles and takes them; 16321 x 257 is 2555 and takes 16-row tiles.
  - Mixed batch: four sizes, a one-pixel second tile column, octave 0 on 32-row tiles and the later octaves on 16-row tiles,
    one image with fewer octaves than the others.
  - Scan: every return of localizeKeypoint, every residue of a 64 x 16 scan tile, both ends of both scan axes, accepted
    extrema after 1 .. 5 Newton steps, walks across a tile edge, claim collisions, equal neighbours that are both extrema,
    negative extrema, the three Hessian point types, windows of width 1 / 64 / 65 / 129 and height 1 / 16 / 17 / 33, L = 5 and 8,
    and a set of more than 1024 accepted extrema.
  - Flush: the 32-image batch has more (image, octave, level) jobs than one launch's table holds, and the reference finds
    keypoints in the octaves that fall behind the flush.
"""
import numpy as np
import pytest

from tests import pyramid_cases as PC


@pytest.fixture(scope="module")
def scans(oracle):
    return {c.name: PC.oracle_scan(oracle, c) for c in PC.SCAN_CASES}


def _exits(oracle, rep):
    return dict(zip(oracle.SCAN_EXITS, np.bincount(rep["exit"], minlength=len(oracle.SCAN_EXITS)).tolist()))


# ---- blur ---------------------------------------------------------------------------------------------------------------------
def test_blur_sigmas_give_every_half_width(oracle):
    assert tuple(oracle.blur_ksize(s) for s in PC.BLUR_SIGMAS) == PC.BLUR_KSIZES == tuple(2 * r + 1 for r in range(1, 9))
    assert oracle.blur_ksize(PC.REFUSED_SIGMA) == 19
    for s in PC.TILE32_BLUR_SIGMAS + PC.TILE16_BLUR_SIGMAS:
        assert s in PC.BLUR_SIGMAS
    # the levels of an octave of the default parameters use R = 4 .. 7, the plain blurs on 32-row tiles the other four
    p = oracle.default_params()
    step = 2.0 ** (1.0 / p.numberOfScales)
    inc = [p.initialSigma * step ** i * np.sqrt(step * step - 1) for i in range(p.numberOfScales + 1)]
    assert sorted(oracle.blur_ksize(float(s)) // 2 for s in inc) == [4, 5, 6, 7]
    assert sorted(oracle.blur_ksize(s) // 2 for s in PC.TILE32_BLUR_SIGMAS) == [1, 2, 3, 8]


def test_small_blur_shapes_straddle_the_tile_edges(modsx):
    assert {c - 64 for c in PC.BLUR_COLS} >= {-1, 0, 1} and {r - 16 for r in PC.BLUR_ROWS} >= {-1, 0, 1}
    assert min(PC.BLUR_COLS) == 2 and min(PC.BLUR_ROWS) == 2            # smaller than the halo of every R (R + 1 >= 2)
    assert max(PC.BLUR_COLS) > 128 and max(PC.BLUR_ROWS) > 32           # three tile columns, three tile rows
    for r in PC.BLUR_ROWS:
        for c in PC.BLUR_COLS:
            assert modsx.blur_geometry([(r, c)]) == (16, PC.tiles([(r, c)], 16))


def test_tile_height_boundary(modsx):
    assert PC.tiles([PC.TILE32_SHAPE], 32) == PC.TILE_BOUNDARY == 5 * 512
    assert PC.tiles([PC.TILE16_SHAPE], 32) == 2555
    assert modsx.blur_geometry([PC.TILE32_SHAPE]) == (32, 2560)
    assert modsx.blur_geometry([PC.TILE16_SHAPE]) == (16, PC.tiles([PC.TILE16_SHAPE], 16))
    # the rule counts the tiles of all jobs of a launch together
    assert modsx.blur_geometry([(32, 64)] * 32) == (16, 64)
    assert modsx.blur_geometry([(2560, 64)] * 31 + [(2528, 64)]) == (16, 2 * (31 * 80 + 79))      # 2559 tiles of 32 rows
    assert modsx.blur_geometry([(2560, 64)] * 32) == (32, 2560)
    with pytest.raises(RuntimeError):
        modsx.blur_geometry([(0, 64)])
    with pytest.raises(RuntimeError):
        modsx.blur_geometry([(8, 8)] * 33)


def test_mixed_batch_shape(modsx, oracle):
    shapes = PC.MIXED_SHAPES
    assert len(set(shapes)) == len(shapes) >= 3 and all(c == 65 for _, c in shapes)
    B = oracle.default_params().border
    octs = [PC.octave_shapes(r, c, B) for r, c in shapes]
    assert sorted(len(o) for o in octs) == [2, 3, 3, 3]
    th, t = modsx.blur_geometry([o[0] for o in octs])
    assert th == 32 and t >= PC.TILE_BOUNDARY and t == PC.tiles(shapes, 32)
    for k in (1, 2):
        live = [o[k] for o in octs if len(o) > k]
        assert modsx.blur_geometry(live)[0] == 16
    assert len([o for o in octs if len(o) > 2]) == 3                     # the batch shrinks at the last octave
    assert sum(r * c for r, c in shapes) < 2.8e6


# ---- scan ---------------------------------------------------------------------------------------------------------------------
def test_every_exit_of_the_walk_is_reached(oracle, scans):
    total = {k: 0 for k in oracle.SCAN_EXITS}
    for name, s in scans.items():
        e = _exits(oracle, s["report"])
        print(name, e)
        assert e["claimed"] == 0
        for k, v in e.items():
            total[k] += v
    assert all(v >= 1 for k, v in total.items() if k != "claimed"), total
    b1 = _exits(oracle, scans["border1"]["report"])
    assert min(b1[k] for k in ("border_right", "border_bottom", "border_left", "border_top")) >= 1
    b2 = _exits(oracle, scans["border2"]["report"])
    assert sum(b2[k] >= 1 for k in ("border_right", "border_bottom", "border_left", "border_top")) >= 3
    n5 = _exits(oracle, scans["noise5"]["report"])
    assert min(n5[k] for k in ("edge_high", "edge_negative", "offset", "value")) >= 1
    assert _exits(oracle, scans["noise5_mode4"]["report"])["value"] == 0     # thresholds of mode 4 are 0
    assert _exits(oracle, scans["plateau"]["report"])["nan"] >= 30


@pytest.mark.parametrize("name", ["noise5", "noise5_mode4", "noise8"])
def test_noise_planes_cover_the_scan_tile(scans, name):
    case, acc = PC.scan_case(name), scans[name]["accepted"]
    L, rows, cols = case.planes()[0].shape
    B = case.border
    assert {int(x) for x in (acc["c0"] - B) % 64} == set(range(64))
    assert {int(x) for x in (acc["r0"] - B) % 16} == set(range(16))
    assert (acc["r0"] == B).any() and (acc["r0"] == rows - B - 1).any() and (acc["c0"] == B).any() and (acc["c0"] == cols - B - 1).any()
    assert set(acc["level"].tolist()) == set(range(1, L - 1))
    assert set(acc["iters"].tolist()) == {1, 2, 3, 4, 5}
    moved = (acc["r0"] != acc["r"]) | (acc["c0"] != acc["c"])
    cross = ((acc["r0"] - B) // 16 != (acc["r"] - B) // 16) | ((acc["c0"] - B) // 64 != (acc["c"] - B) // 64)
    assert moved.sum() >= 20 and cross.sum() >= 1
    assert (acc["val"] < 0).sum() >= 100 and set(acc["type"].tolist()) == {0, 1, 2}
    assert (cols - 2 * B + 63) // 64 >= 3 and (rows - 2 * B + 15) // 16 >= 3       # more than one tile each way


def test_claim_collisions_and_the_large_set(oracle, scans):
    big = scans[PC.BIG]
    assert len(big["accepted"]) > 1024
    assert len(scans["plateau"]["accepted"]) < 1024 // 4                           # the "following smaller call"
    for name, least in (("noise5", 140), ("noise5_mode4", 100), ("noise8", 140)):
        s = scans[name]
        lost = _exits(oracle, s["report_claim"])["claimed"]
        assert lost >= least and lost == len(s["accepted"]) - len(s["kp"])
        # a collision is two accepted extrema that end on one pixel: the later one in (level, row, column) order loses
        key = s["accepted"]["r"].astype(np.int64) * 100000 + s["accepted"]["c"]
        assert len(key) - len(np.unique(key)) == lost


def test_plateau_plants(oracle, scans):
    resp, _ = PC.scan_case("plateau").planes()
    rep = scans["plateau"]["report"]
    where = {(int(e["level"]), int(e["r0"]), int(e["c0"])): e for e in rep}
    for a, b, v in PC.EQUAL_PAIRS:
        assert resp[a] == resp[b] == np.float32(v)
        assert a in where and b in where                                            # both equal neighbours are extrema
        assert where[a]["exit"] == 0 and where[b]["exit"] == 0
    acc = scans["plateau"]["accepted"]
    assert (acc["val"] < 0).any() and (acc["val"] > 0).any()
    nan = rep[rep["exit"] == oracle.SCAN_EXITS.index("nan")]
    assert (nan["iters"] == 1).all()
    blk = PC.NAN_BLOCK
    assert ((nan["r0"] >= blk[1].start) & (nan["r0"] < blk[1].stop) & (nan["c0"] >= blk[2].start) & (nan["c0"] < blk[2].stop)).all()


def test_window_sizes(scans):
    widths, heights = set(), set()
    for (r, c) in PC.WINDOW_SHAPES:
        name = "window_%dx%d" % (r - 10, c - 10)
        case = PC.scan_case(name)
        assert case.border == 5 and case.planes()[0].shape == (5, r, c)
        widths.add(c - 10); heights.add(r - 10)
        acc = scans[name]["accepted"]
        assert len(acc) >= 1, name
        assert acc["r0"].min() >= 5 and acc["r0"].max() <= r - 6 and acc["c0"].min() >= 5 and acc["c0"].max() <= c - 6
    assert widths == {1, 64, 65, 129} and heights == {1, 16, 17, 33}
    # last column of a 65-wide window: the one pixel of the second tile column; row 16 of a 17-row window likewise
    assert (scans["window_17x65"]["accepted"]["c0"] == 69).any() and (scans["window_17x65"]["accepted"]["r0"] == 21).any()


def test_both_scan_kernels_have_cases():
    Ls = {c.L for c in PC.SCAN_CASES}
    assert Ls == {5, 8}
    assert sum(c.L == 5 for c in PC.SCAN_CASES) >= 10


def test_oracle_scan_agrees_with_the_oracle_pyramid(oracle, small_pair):
    """orc_scan_levels on the planes orc_octave_levels builds gives the first octave's keypoints of orc_detect_scalespace: the
    report variant is the code path of the detector, not a restatement."""
    img = small_pair[0]
    p = oracle.default_params()
    first = oracle.gaussian_blur(img, float(np.sqrt(np.float32(p.initialSigma) ** 2 - 0.25)))
    blurs, resps = oracle.octave_levels(first, p)
    kp, rep = oracle.scan_levels(resps, blurs, p, claim=True)
    ref = oracle.detect_scalespace(img, p)
    ref = ref[ref["octave"] == 0]
    assert len(ref) >= 20 and len(kp) == len(ref)
    for f in PC.SSKP_FIELDS:
        assert np.array_equal(kp[f], ref[f]), f
    assert (rep["exit"] == 0).sum() == len(kp)
    with pytest.raises(ValueError):
        oracle.scan_levels(resps, blurs, oracle.default_params(border=0))
    with pytest.raises(ValueError):
        oracle.scan_levels(resps[:4], blurs[:4], p)


def test_scan_mismatches_notices_a_wrong_field(scans):
    """the comparison the GPU module uses accepts the oracle's own answer (in any order) and names what differs"""
    ref = scans["noise5"]
    cand = np.zeros(len(ref["accepted"]), np.dtype([(f, "i4") for f in ("img", "octave", "level", "type", "r0", "c0", "r", "c")]
                                                   + [(f, "f4") for f in ("b0", "b1", "b2", "val")]))
    for f in PC.CAND_FIELDS + ("b0", "b1", "b2", "val"):
        cand[f] = ref["accepted"][f]
    shuffled = cand[np.random.RandomState(0).permutation(len(cand))]
    assert PC.scan_mismatches(shuffled, ref["kp"], ref) == []
    wrong = shuffled.copy()
    wrong["b1"][7] = np.nextafter(wrong["b1"][7], np.float32(9))
    assert PC.scan_mismatches(wrong, ref["kp"], ref) == ["candidate field b1 (bits)"]
    assert PC.scan_mismatches(shuffled[1:], ref["kp"], ref) != []
    assert PC.scan_mismatches(shuffled, ref["kp"][:-1], ref) != []


# ---- flush ----------------------------------------------------------------------------------------------------------------------
def test_flush_batch_fills_the_job_table(oracle):
    B, S = PC.FLUSH_PARAMS["border"], PC.FLUSH_PARAMS["numberOfScales"]
    assert len(PC.FLUSH_SHAPES) == 32
    octs = [PC.octave_shapes(r, c, B) for r, c in PC.FLUSH_SHAPES]
    assert all(len(o) == 7 for o in octs)
    total, flushed = PC.flush_jobs()
    assert total == 32 * 7 * S == 1344 > PC.NMS_MAXJ
    assert flushed == 170 * S                     # five whole octaves and ten images of the sixth: one launch before the last
    # the reference finds keypoints behind the flush: octave 5 of the images from the eleventh on, octave 6 of all
    p = oracle.default_params(**PC.FLUSH_PARAMS)
    imgs = PC.flush_batch()
    behind = 0
    for i in (0, 12, 31):
        kp = oracle.detect_scalespace(imgs[i], p)
        behind += int(((kp["octave"] == 6) | ((kp["octave"] == 5) & (i >= 10))).sum())
    assert behind >= 1
