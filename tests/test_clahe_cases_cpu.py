"""CPU: what the CLAHE case list (tests/clahe_cases.py) reaches, shown with the model (tests/clahe_model.py), and the library's
host-side geometry (mods_amd.clahe_geometry, the function the launcher itself calls) against the model's.  No device."""
import numpy as np
import pytest

from tests import clahe_cases as CC
from tests import clahe_model as M


def _cases(**want):
    return [k for k, c in enumerate(CC.CASES) if all(c[f] == v for f, v in want.items())]


def test_shapes_grids_clips_and_variants_all_occur():
    shapes = {c["shape"] for c in CC.CASES}
    for s in [(2, 2), (8, 8), (9, 17), (64, 64), (100, 75), (135, 239), (131, 257), (768, 1024), CC.ONE_STRIP, CC.TWO_STRIPS]:
        assert s in shapes, s
    assert {c["grid"] for c in CC.CASES} >= {(8, 8), (1, 1), (3, 5), (16, 16)}
    assert {c["clip"] for c in CC.CASES} >= {4.0, 40.0, 0.0, 0.01, 2.5}
    assert {c["variant"] for c in CC.CASES} == {0, 1}
    assert {c["kind"] for c in CC.CASES} == set(CC.CONTENTS)
    # every case has its twin in the other variant, except the three big ones
    twins = {(c["shape"], c["kind"], c["clip"], c["grid"], c["seed"]) for c in CC.CASES if c["variant"] == 1 and c["shape"] != CC.BIG}
    assert twins == {(c["shape"], c["kind"], c["clip"], c["grid"], c["seed"]) for c in CC.CASES if c["variant"] == 0 and c["shape"] != CC.BIG}


def test_geometry_of_the_named_shapes():
    g = M.geometry(2, 2, 4.0, (8, 8))
    assert (g["tile_w"], g["tile_h"], g["pad_cols"], g["pad_rows"]) == (1, 1, 8, 8)      # 6 padded columns of a 2-pixel row
    assert [M.reflect101(p, 2) for p in range(8)] == [0, 1, 0, 1, 0, 1, 0, 1]            # repeated reflections
    g = M.geometry(8, 8, 4.0, (16, 16))
    assert (g["tile_w"], g["pad_cols"]) == (1, 16) and M.reflect101(15, 8) == 1          # 15 -> -1 -> 1: two reflections
    g = M.geometry(8, 8, 4.0, (8, 3))
    assert (g["pad_cols"], g["pad_rows"]) == (16, 9)                                      # the divisible side gets a whole grid
    assert _cases(shape=(8, 8), grid=(8, 3)) and _cases(shape=(8, 8), grid=(16, 16))
    g = M.geometry(8, 8, 4.0, (8, 8))
    assert (g["tile_w"], g["tile_h"], g["pad_cols"], g["pad_rows"]) == (1, 1, 8, 8)      # divisible both ways: no padding
    g = M.geometry(135, 239, 4.0, (8, 8))
    assert (g["tile_w"], g["tile_h"]) == (30, 17) and g["lut_scale"] == np.float32(0.5)   # 510 px: every odd sum is a tie
    g = M.geometry(64, 64, 0.01, (8, 8))
    assert g["clip_limit"] == 1                                                            # (int)(0.01 * 64 / 256) = 0, raised to 1
    assert M.geometry(64, 64, 0.0, (8, 8))["clip_limit"] == 0
    assert M.geometry(768, 1024, 4.0, (8, 8))["clip_limit"] == 192


def test_lut_rounding_ties_occur_at_half_scale():
    k = _cases(shape=(135, 239), kind="noise", clip=0.0, variant=0)[0]
    e = CC.expected(k)
    sums = np.cumsum(e["hist"], axis=1)
    odd = (sums % 2 == 1)
    assert odd.sum() > 1000
    assert np.array_equal(e["lut"][odd], (np.minimum(2 * np.rint(sums[odd] / 4.0), 255)).astype(np.uint8))   # x.5 goes to the even neighbour


def test_source_conversion_of_the_f32_edge_values():
    vals = np.array([0.5, 1.5, 2.5, 3.5, 254.5, 255.5, -0.5, -3.0, -1e30, 255.49, 256.0, 1e30, np.nan, np.inf, -np.inf], np.float32)
    assert M.to_u8(vals).tolist() == [0, 2, 2, 4, 254, 255, 0, 0, 0, 255, 255, 255, 0, 255, 0]
    for k in _cases(kind="f32_edges"):
        img = CC.image(k)
        if img.size < 1000:
            continue
        with np.errstate(invalid="ignore"):
            fr = img - np.floor(img)
            assert ((fr == 0.5) & (np.floor(img) % 2 == 0)).any() and ((fr == 0.5) & (np.floor(img) % 2 == 1)).any()
            assert (img < 0).any() and (img > 255).any() and np.isnan(img).any() and np.isinf(img).any()


def test_contents_reach_the_clipping_paths():
    residuals, small_clipped, unclipped_tiles = set(), 0, 0
    for k in range(len(CC.CASES)):
        e = CC.expected(k)
        if e["geo"]["clip_limit"] == 0:
            assert not e["clipped"].any()
            continue
        hit = e["clipped"] > 0
        residuals |= set(int(r) for r in e["residual"][hit])
        small_clipped += int(((e["clipped"] > 0) & (e["clipped"] < 256)).sum())
        unclipped_tiles += int((~hit).sum())
    assert {0, 1, 255} <= residuals
    assert small_clipped > 0 and unclipped_tiles > 0
    # the constant image: one bin holds the tile, everything above the limit is spread
    k = _cases(shape=(64, 64), kind="constant", clip=0.01, grid=(1, 1), variant=0)[0]
    e = CC.expected(k)
    assert e["clipped"][0] == 4095 and e["residual"][0] == 255 and (e["hist"][0] > 0).sum() == 1
    # a saturated tile beside flat ones
    k = _cases(shape=(64, 64), kind="saturated_tile", variant=0)[0]
    e = CC.expected(k)
    assert e["hist"][0][255] == 64 and e["hist"][1][100] == 64


def test_an_interpolated_value_lands_on_a_half():
    k = _cases(shape=(64, 64), kind="noise", grid=(8, 8), seed=CC.TIE_SEED, variant=0)[0]
    e = CC.expected(k)
    tie = (e["res"] - np.floor(e["res"])) == 0.5
    assert tie.sum() > 100
    odd = tie & (np.floor(e["res"]) % 2 == 1)
    even = tie & (np.floor(e["res"]) % 2 == 0)
    assert odd.any() and even.any()
    assert np.array_equal(e["out"][odd], (np.floor(e["res"][odd]) + 1).astype(np.uint8))      # up to the even value
    assert np.array_equal(e["out"][even], np.floor(e["res"][even]).astype(np.uint8))           # down to it


def test_the_variants_differ_in_each_of_their_three_places():
    lut_differs = axis_differs = formula_differs = out_differs = 0
    for k in _cases(variant=0):
        c = CC.CASES[k]
        if c["shape"] == CC.BIG:
            continue
        e0 = CC.expected(k)
        twin = [j for j in _cases(variant=1, shape=c["shape"], kind=c["kind"], clip=c["clip"], grid=c["grid"], seed=c["seed"])]
        e1 = CC.expected(twin[0])
        assert np.array_equal(e0["hist"], e1["hist"])
        lut_differs += int((e0["lut"] != e1["lut"]).any())                                        # (a) the residual's spread
        a0 = M.axis_terms(c["shape"][1], e0["geo"]["tile_w"], c["grid"][0], 0)
        a1 = M.axis_terms(c["shape"][1], e0["geo"]["tile_w"], c["grid"][0], 1)
        axis_differs += int(any((p != q).any() for p, q in zip(a0, a1)))                          # (b) x / tileW against x * (1 / tileW)
        o0, _ = M.apply_luts(e0["u8"], e0["lut"], e0["geo"], c["grid"], 0, formula=0)
        o1, _ = M.apply_luts(e0["u8"], e0["lut"], e0["geo"], c["grid"], 0, formula=1)
        formula_differs += int((o0 != o1).any())                                                  # (c) the order of the sum
        out_differs += int((e0["out"] != e1["out"]).any())
    assert lut_differs > 0 and axis_differs > 0 and formula_differs > 0 and out_differs > 0


def test_batch_list_is_mixed():
    shapes = [CC.CASES[k]["shape"] for k in CC.BATCH]
    assert len(set(shapes)) == len(shapes) >= 8 and CC.BIG in shapes and (2, 2) in shapes


# ------------------------------------------------------------------------------------------ the library's host geometry
def test_library_geometry_equals_the_models(modsx):
    seen = set()
    extra = [((s, g, c)) for s in [(1, 1), (1, 7), (7, 1), (16384, 4096), (4096, 16384), (1080, 1920), (13, 16384)] for g in CC.GRIDS + [(256, 1), (1, 256)]
             for c in (4.0, 0.0)]
    for shape, grid, clip in [(c["shape"], c["grid"], c["clip"]) for c in CC.CASES] + extra:
        if (shape, grid, clip) in seen:
            continue
        seen.add((shape, grid, clip))
        got = modsx.clahe_geometry(shape[0], shape[1], clip, grid)
        ref = M.geometry(shape[0], shape[1], clip, grid)
        for f in ("tile_w", "tile_h", "pad_cols", "pad_rows", "clip_limit"):
            assert got[f] == ref[f], (shape, grid, clip, f)
        assert got["lut_scale"].tobytes() == ref["lut_scale"].tobytes(), (shape, grid)
        # the work split: whole rows of a tile per strip, at most 4096 px unless a single row is longer; at most 256 strips
        assert 1 <= got["strip_rows"] <= got["tile_h"] and got["strips"] == -(-got["tile_h"] // got["strip_rows"]) <= 256
        if got["strips"] > 1 and got["tile_h"] <= 256 * max(1, 4096 // got["tile_w"]):
            assert got["strip_rows"] == max(1, 4096 // got["tile_w"])
        assert got["apply_blocks"] == -(-shape[0] * shape[1] // 4096)


def test_strip_rule_boundaries(modsx):
    """for each launch one shape with exactly one piece of work per tile / image and one just above"""
    one = modsx.clahe_geometry(CC.ONE_STRIP[0], CC.ONE_STRIP[1], 4.0, (1, 1))
    two = modsx.clahe_geometry(CC.TWO_STRIPS[0], CC.TWO_STRIPS[1], 4.0, (1, 1))
    assert (one["strips"], one["apply_blocks"]) == (1, 1) and one["tile_w"] * one["tile_h"] == 4096
    assert (two["strips"], two["apply_blocks"]) == (2, 2) and two["tile_h"] == one["tile_h"] + 1
    assert _cases(shape=CC.ONE_STRIP, grid=(1, 1)) and _cases(shape=CC.TWO_STRIPS, grid=(1, 1))
    big = modsx.clahe_geometry(768, 1024, 4.0, (8, 8))
    assert (big["tile_w"], big["tile_h"], big["strips"], big["strip_rows"], big["apply_blocks"]) == (128, 96, 3, 32, 192)
    assert modsx.clahe_geometry(768, 1024, 40.0, (1, 1))["strips"] == 192
    assert modsx.clahe_geometry(16384, 4096, 4.0, (1, 1))["strips"] == 256        # the cap: 64 rows per strip


@pytest.mark.parametrize("kw", [dict(tiles=(0, 8)), dict(tiles=(8, 0)), dict(tiles=(-1, 8)), dict(tiles=(17, 16)), dict(tiles=(257, 1)),
                                dict(clip_limit=-1.0), dict(clip_limit=float("nan")), dict(clip_limit=float("inf")), dict(variant=2),
                                dict(variant=-1)])
def test_geometry_refusals(modsx, kw):
    with pytest.raises(RuntimeError):
        modsx.clahe_geometry(64, 64, **kw)


def test_geometry_size_refusals(modsx):
    for rows, cols in [(0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385), (16384, 8192)]:
        with pytest.raises(RuntimeError, match="image size"):
            modsx.clahe_geometry(rows, cols)
    modsx.clahe_geometry(16384, 4096)
    assert modsx.clahe_geometry(64, 64, tiles=(16, 16))["tile_w"] == 4        # 256 tiles: the limit itself is accepted
    assert modsx.clahe_geometry(64, 64, clip_limit=1e300)["clip_limit"] == 2 ** 31 - 1
