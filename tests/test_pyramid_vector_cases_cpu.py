"""CPU: the shapes of the pyramid vector-tile suite (tests/pyramid_vector_cases.py) reach what
tests/test_gpu_pyramid_vector_tiles.py relies on.  The conditions are conditions on the rules restated there (which group of the
tile fill is one 16-byte load, which block of the resize is full), on the oracle and on the library's host-only tile rule.

  - Fill rule: a tile filled by the rule is the BORDER_REPLICATE tile, for every R, on tiles of every kind.
  - For every R some tile's fill is all-vector: the middle tile column of 197 columns (R = 8 loads columns 55 .. 138, so it
    needs cols >= 139).  131 columns never qualify: their second tile column loads up to column 132 at least, so it is one of
    the tiles that mix on the right edge.
  - Tiles that mix vector and scalar groups on the left edge, and on the right edge; a vector group that starts on the border
    column; groups that straddle either border; shapes without any vector group (1 and 3 columns; the library
    takes no image with a side of one pixel, so on the GPU it is 3 columns); 5 columns hold a vector
    group for R = 2, 3, 6, 7 only, 8 columns for every R.
  - Row pairs that clamp to one image row, at the top, at the bottom and for the one-row image (which the library refuses: the GPU
    module requires that refusal and meets the clamped pairs at the top and bottom of 3, 18 and 35 rows).
  - Last tile columns of 62, 3 and 5 pixels; planes at odd dword offsets (odd rows x odd columns).
  - Resize: a partial bottom row, a partial right column, rings that cross a tile column and a tile row, three tile columns; the
    block rule equals the oracle's resize bit for bit.
"""
import numpy as np
import pytest

from tests import pyramid_cases as PC
from tests import pyramid_vector_cases as VC


def test_sigmas_are_the_half_widths(oracle):
    assert tuple(oracle.blur_ksize(s) // 2 for s in PC.BLUR_SIGMAS) == VC.HALF_WIDTHS


def test_every_shape_takes_16_row_tiles(modsx):
    for r in VC.BLUR_ROWS:
        for c in VC.BLUR_COLS:
            if VC.uploadable(r, c):
                assert modsx.blur_geometry([(r, c)])[0] == 16
            else:                                     # a side of one pixel: the library takes no such image (capi.hip image_size_ok)
                with pytest.raises(RuntimeError):
                    modsx.blur_geometry([(r, c)])
    for s in VC.OCTAVE_SHAPES:
        assert modsx.blur_geometry([s])[0] == 16
    assert modsx.blur_geometry(list(VC.PYRAMID_SHAPES))[0] == 16


@pytest.mark.parametrize("R", VC.HALF_WIDTHS)
def test_fill_rule_gives_the_replicated_tile(R):
    for rows, cols in ((35, 197), (3, 5), (1, 1), (18, 67), (17, 62), (35, 131)):
        img = VC.blur_image(R, rows, cols)
        for ty0 in VC.tile_origins(rows, 16):
            for tx0 in VC.tile_origins(cols, VC.TW):
                assert np.array_equal(VC.fill_tile(img, R, 16, tx0, ty0), VC.replicated_tile(img, R, 16, tx0, ty0)), (rows, cols, tx0, ty0)


def test_tile_dims():
    for R in VC.HALF_WIDTHS:
        sh, sw, SW = VC.tile_dims(R, 16)
        assert sh % 2 == 0 and SW % 4 == 0 and sw <= SW <= sw + 2 and sw == 66 + 2 * R + 2
        assert len(VC.fill_groups(R, 197, 64)) == SW // 4


@pytest.mark.parametrize("R", VC.HALF_WIDTHS)
def test_an_all_vector_tile_for_every_half_width(R):
    assert 197 in VC.BLUR_COLS and 197 in [c for _, c in VC.OCTAVE_SHAPES]
    assert VC.fill_kind(R, 197, 64) == "vector"
    first, last = VC.fill_groups(R, 197, 64)[0][0], VC.fill_groups(R, 197, 64)[-1][0] + 3
    assert first == 63 - R and first >= 0 and last <= 196
    if R == 8:
        assert (first, last) == (55, 138)
        assert VC.fill_kind(8, 139, 64) == "vector" and VC.fill_kind(8, 138, 64) == "mixed"
    # 131 columns: the second tile column reaches past the last column for every R
    assert last >= 132 and VC.fill_kind(R, 131, 64) == "mixed"


@pytest.mark.parametrize("R", VC.HALF_WIDTHS)
def test_mixed_tiles_on_both_edges(R):
    for cols in (62, 67, 131, 197):
        g = VC.fill_groups(R, cols, 0)
        assert VC.fill_kind(R, cols, 0) == "mixed" and not g[0][1]                 # left edge: the first groups are scalar
    for cols in (131, 197):
        g = VC.fill_groups(R, cols, 64 * ((cols - 1) // 64))
        assert g[0][1] and not g[-1][1]                                            # right edge: vector first, scalar last
    # one tile with both edges: scalar, vector, scalar
    g = [v for _, v in VC.fill_groups(R, 62, 0)]
    assert not g[0] and not g[-1] and any(g)


def test_groups_on_the_border_columns():
    starts_on_border, straddle_left, straddle_right, outside_left, outside_right = set(), set(), set(), set(), set()
    for R in VC.HALF_WIDTHS:
        for cols in VC.BLUR_COLS:
            for tx0 in VC.tile_origins(cols, VC.TW):
                for gx0, vec in VC.fill_groups(R, cols, tx0):
                    if gx0 == 0 and vec:
                        starts_on_border.add(R)
                    if gx0 < 0 <= gx0 + 3:
                        straddle_left.add(R); assert not vec
                    if gx0 <= cols - 1 < gx0 + 3:
                        straddle_right.add((R, cols)); assert not vec
                    if gx0 + 3 < 0:
                        outside_left.add(R); assert not vec
                    if gx0 > cols - 1:
                        outside_right.add(R); assert not vec
                    if gx0 + 3 == cols - 1 and gx0 >= 0:
                        assert vec                                                 # the last group that is still whole
    assert starts_on_border == {3, 7}                                              # -1 - R + 4 g == 0
    assert straddle_left == {1, 2, 4, 5, 6, 8}
    assert outside_left == {3, 4, 5, 6, 7, 8} and outside_right == set(VC.HALF_WIDTHS)
    assert {R for R, _ in straddle_right} == set(VC.HALF_WIDTHS)
    # the octave shapes: R = 4 .. 7 of the default levels see a first group on the border column and partial last groups
    assert sorted(c % 4 for _, c in VC.OCTAVE_SHAPES) == [1, 2, 3, 3]
    for R in (4, 5, 6, 7):
        for _, cols in VC.OCTAVE_SHAPES:
            assert VC.fill_kind(R, cols, 0) == "mixed"
    assert any(gx0 == 0 and vec for gx0, vec in VC.fill_groups(7, 67, 0))


def test_narrow_shapes():
    for R in VC.HALF_WIDTHS:
        assert VC.fill_kind(R, 1, 0) == "scalar" and VC.fill_kind(R, 3, 0) == "scalar"
        n5 = sum(v for _, v in VC.fill_groups(R, 5, 0))
        assert n5 == (1 if R in (2, 3, 6, 7) else 0)
        n8 = sum(v for _, v in VC.fill_groups(R, 8, 0))
        assert n8 == (2 if R % 4 == 3 else 1)                                      # columns 0 .. 3 and 4 .. 7, or one group inside
    assert {c % 64 for c in VC.BLUR_COLS if c > 8} == {62, 3, 5}                 # last tile columns of 62, 3 and 5 pixels


def test_row_pairs_that_clamp_to_one_row():
    for R in VC.HALF_WIDTHS:
        one = VC.pair_rows(R, 16, 1, 0)
        assert all(a == b == 0 for a, b in one)                                    # the one-row image: every pair
        top = VC.pair_rows(R, 16, 35, 0)
        assert top[0] == (0, 0) and any(a + 1 == b for a, b in top)
        bottom = VC.pair_rows(R, 16, 35, 32)                                       # the last tile row holds three image rows
        assert bottom[-1] == (34, 34) and any(a + 1 == b for a, b in bottom)
        # odd R: a pair straddles the first image row (tile rows -1 and 0 both read row 0 ... row 0 and 1 do not)
        assert ((0, 0) in top) and ((0, 1) in top or (1, 2) in top)
    assert 1 in VC.BLUR_ROWS and 35 in VC.BLUR_ROWS


def test_planes_at_odd_dword_offsets():
    odd = [(r, c) for r in VC.BLUR_ROWS for c in VC.BLUR_COLS if r % 2 and c % 2]
    assert len(odd) >= 12
    # rows of such a plane start at every residue of 4 dwords
    assert {(y * 67) % 4 for y in range(35)} == {0, 1, 2, 3} and {(y * 197) % 4 for y in range(35)} == {0, 1, 2, 3}
    # the levels of an octave lie one after the other: a level of odd size puts the next at an odd offset
    assert [r * c % 2 for r, c in VC.OCTAVE_SHAPES] == [1, 0, 1, 0]


# ---- resize -------------------------------------------------------------------------------------------------------------------
def _octaves(oracle, shape):
    return PC.octave_shapes(shape[0], shape[1], oracle.default_params().border)


def test_pyramid_batch_octaves(oracle):
    octs = [_octaves(oracle, s) for s in VC.PYRAMID_SHAPES]
    assert [len(o) for o in octs] == [2, 2, 2, 3]
    assert [o[1] for o in octs] == [(22, 34), (24, 66), (23, 66), (48, 130)]
    assert octs[3][2] == (24, 65)
    for o in octs:
        for (sr, sc), (dr, dc) in zip(o, o[1:]):
            assert (dr, dc) == (VC.half(sr), VC.half(sc))


def test_resize_shapes_reach_the_partial_blocks_and_the_rings(oracle):
    kinds = {}
    for s in VC.PYRAMID_SHAPES:
        o = _octaves(oracle, s)
        for (sr, sc), (dr, dc) in zip(o, o[1:]):
            for dy in range(dr):
                for dx in range(dc):
                    kinds.setdefault((sr, sc), set()).add(VC.block_kind(sr, sc, dx, dy))
    # 47 rows -> 24: the last destination row has one source row; 131 columns -> 66: the last column has one source column
    assert VC.block_kind(47, 133, 10, 23) == "partial" and VC.block_kind(47, 133, 10, 22) == "full"
    assert VC.block_kind(46, 131, 65, 10) == "partial" and VC.block_kind(46, 131, 64, 10) == "full"
    assert VC.block_kind(95, 259, 129, 47) == "partial"                            # both at once: a single source pixel
    assert kinds[(45, 67)] == {"full"} or kinds[(45, 67)] == {"full", "partial"}
    assert all("zero" not in k for k in kinds.values())                           # cvRound never asks for a block outside the source
    # 66 destination columns: the second tile column holds two pixels and takes its ring's column 63 from the first;
    # 130: three tile columns; 23, 24 and 48 rows: rings that cross a tile row
    assert (66 + 63) // 64 == 2 and (130 + 63) // 64 == 3
    ring = VC.ring_entries(24, 66, 64, 8)
    assert (8, 63) in ring and (7, 63) in ring and (16, 65) in ring and (7, 64) in ring
    assert all(0 <= y < 24 and 0 <= x < 66 for y, x in ring)
    assert (8, 66) not in ring                                                     # outside the destination: never formed
    ring0 = VC.ring_entries(24, 66, 0, 0)
    assert (0, 64) in ring0 and (8, 0) in ring0 and all(y >= 0 and x >= 0 for y, x in ring0)
    last = VC.ring_entries(23, 66, 64, 16)                                         # 23 rows: a last tile row of 7
    assert (15, 64) in last and all(y < 23 for y, _ in last)


def test_block_rule_is_the_oracles_resize(oracle):
    for i, s in enumerate(VC.PYRAMID_SHAPES + ((7, 9), (2, 3), (13, 64))):
        src = PC.image(s[0], s[1], 900 + i) + np.float32(0.25) * PC.image(s[0], s[1], 950 + i)
        assert np.array_equal(VC.resize_by_rule(src), oracle.resize_half(src)), s
