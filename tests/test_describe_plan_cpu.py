"""CPU: the planner of the description stage (mods_amd/csrc/describe_plan.cpp) on its own, through mods_amd.describe_plan
(modsx_debug_describe_plan: no device, no context).

What the GPU modules read back from a device call's counters is proven here from the plan alone: the path class of every window
size of tests/describe_cases.py, both sides of every class change, the numbers of distinct row-tile and column-tile counts
(ROW_TILE_VALUES, COL_TILE_VALUES: first read off an MI355X, here from the planner), the direct branch, the refusal of a 513-tap
window and its counting rule, the call without regions, and the chunk cuts of the crafted and the views case against
describe_cases.greedy_cuts, the independent restatement of the rule.  tests/test_gpu_describe_paths.py and
tests/test_gpu_describe_chunks.py assert that a device call books exactly what this plan says.
"""
import numpy as np
import pytest

from tests import describe_cases as DC

ERR_ARG = -1     # include/modsx.h: MODSX_ERR_ARG
ZERO = dict.fromkeys(DC.PER_WINDOW, 0)


def _plan(modsx, regs, mr_size=DC.MR_SIZE, **kw):
    p = modsx.describe_plan(regs, mr_size, **kw)
    assert p["rc"] == 0 and p["error"] == "", p
    return p["counters"], p["cuts"]


@pytest.fixture(scope="module")
def sweep(modsx):
    """{P: signature per window} of every size of the list, three regions each"""
    out = {}
    for P in DC.SIZES:
        c, cuts = _plan(modsx, DC.regions_of(P))
        assert (c["calls"], c["chunks"], c["max_chunks"], c["jobs"], c["direct_jobs"]) == (1, 1, 1, 3, 0) and not cuts, (P, c, cuts)
        assert (c["chunks_mid_image"], c["chunks_later_image"]) == (0, 0), (P, c)
        assert all(c[k] % 3 == 0 for k in DC.PER_WINDOW), "P = %d: three windows of one size, three times the tiles: %r" % (P, c)
        out[P] = {k: c[k] // 3 for k in DC.PER_WINDOW}
    return out


def test_every_path_class_and_both_sides_of_every_change(sweep):
    cls = [(P, DC.class_of(sweep[P])) for P in DC.SIZES]
    runs = []
    for P, c in cls:
        if not runs or runs[-1][0] != c:
            runs.append([c, P, P])
        runs[-1][2] = P
    print("path classes over P: %r" % (runs,))
    assert tuple(r[0] for r in runs) == DC.CLASSES, runs
    for a, b in zip(runs, runs[1:]):
        assert b[1] - a[2] == 2, "%s ends at P = %d, %s begins at P = %d" % (a[0], a[2], b[0], b[1])
    for c, P in DC.CLASS_SIZE.items():
        assert dict(cls)[P] == c, "P = %d is %s, not %s" % (P, dict(cls)[P], c)
    rows = {sweep[P]["lds_row_tiles"] for P in DC.SIZES} - {0}
    cols = {sweep[P]["lds_col_tiles"] for P in DC.SIZES} - {0}
    print("row tiles per window: %d values %r\ncolumn tiles per window: %d values %r" % (len(rows), sorted(rows), len(cols), sorted(cols)))
    assert len(rows) == DC.ROW_TILE_VALUES and len(rows) >= 25, sorted(rows)
    assert len(cols) == DC.COL_TILE_VALUES, sorted(cols)
    # k_patch_sample's 64 x 128 tiles: both sides of the 128-column edge, and a ragged edge in both directions
    assert sweep[1023]["sample_tiles"] == 16 * 8 and sweep[1025]["sample_tiles"] == 17 * 9


def test_direct_branch_plans_no_tiles(modsx):
    c, cuts = _plan(modsx, DC.regions_of(0))
    assert (c["calls"], c["chunks"], c["jobs"], c["direct_jobs"]) == (1, 1, 3, 3) and not cuts, c
    assert {k: c[k] for k in DC.PER_WINDOW} == ZERO, c
    # fast extraction: every region takes the direct branch, whatever its size
    c, _ = _plan(modsx, DC.regions_of(63), fast=1)
    assert (c["jobs"], c["direct_jobs"]) == (3, 3) and {k: c[k] for k in DC.PER_WINDOW} == ZERO, c


def test_window_with_513_taps_is_refused_and_counted_as_an_empty_chunk(modsx):
    p = modsx.describe_plan(DC.regions_of(DC.REFUSED_P), DC.MR_SIZE)
    assert p["rc"] == ERR_ARG and "descriptor window too large" in p["error"], p
    c = p["counters"]
    assert (c["calls"], c["chunks"], c["jobs"], c["max_chunks"]) == (1, 1, 0, 0), c
    assert {k: c[k] for k in DC.PER_WINDOW} == ZERO and not p["cuts"], p
    # the last size accepted, and the planner as usable as before
    assert _plan(modsx, DC.regions_of(2329))[0]["jobs"] == 3


def test_call_without_regions_is_a_call_with_no_chunk(modsx):
    empty = DC.regions_of(19)[:0]
    for regs in ([], empty, [empty, empty]):
        c, cuts = _plan(modsx, regs)
        assert (c["calls"], c["chunks"], c["max_chunks"], c["jobs"]) == (1, 0, 0, 0) and not cuts, c


def test_crafted_image_is_cut_where_the_rule_says(modsx):
    regs = DC.crafted_regions()
    windows = [DC.window_of(s) for s in regs["det_kp"]["s"]]
    c, cuts = _plan(modsx, regs, arena_floats=DC.ARENA_FLOOR_FLOATS)
    assert cuts == [42, 60, 81, 123] == DC.greedy_cuts(windows), cuts
    assert (c["calls"], c["chunks"], c["max_chunks"], c["chunks_mid_image"], c["chunks_later_image"]) == (1, 5, 5, 4, 0), c
    assert c["jobs"] == len(regs) and c["direct_jobs"] == windows.count(0)
    assert c["sample_tiles"] == ((2083 + 63) // 64) * ((2083 + 127) // 128), c
    one, none = _plan(modsx, regs)                       # the default arena of 192 MiB
    assert (one["chunks"], one["chunks_mid_image"]) == (1, 0) and not none
    assert {k: one[k] for k in ("jobs", "direct_jobs") + DC.PER_WINDOW} == {k: c[k] for k in ("jobs", "direct_jobs") + DC.PER_WINDOW}


def test_views_case_is_cut_where_the_rule_says_however_it_is_split_into_images(modsx, oracle, small_pair):
    regs, _ = DC.views_case(oracle, small_pair[0])      # as in tests/test_describe_cases_cpu.py
    windows = [DC.window_of(s, DC.VIEWS_DESC_MR) for s in regs["det_kp"]["s"]]
    want = DC.greedy_cuts(windows)
    # the regions of a view: the identity carries img_id 0, view v > 0 carries v
    starts = [i for i in range(1, len(regs)) if regs["img_id"][i] != regs["img_id"][i - 1]]
    views = np.split(regs, starts)
    assert len(views) == 11
    c11, cuts11 = _plan(modsx, views, DC.VIEWS_DESC_MR, arena_floats=DC.ARENA_FLOOR_FLOATS)
    c1, cuts1 = _plan(modsx, regs, DC.VIEWS_DESC_MR, arena_floats=DC.ARENA_FLOOR_FLOATS)
    print("views: %d regions, cuts %r, views begin at %r\nas 11 images %r\nas one list  %r" % (len(regs), cuts11, [0] + starts, c11, c1))
    assert cuts11 == want and cuts1 == want
    # the thresholds the small-arena child of tests/test_gpu_describe_chunks.py must show
    assert c11["chunks"] == len(want) + 1 >= 4 and c11["chunks_mid_image"] >= 3 and c11["chunks_later_image"] >= 1, c11
    assert c11["chunks_mid_image"] == sum(k not in starts for k in want)
    assert (c1["chunks"], c1["chunks_mid_image"], c1["chunks_later_image"]) == (len(want) + 1, len(want), 0), c1
    same = ("jobs", "direct_jobs") + DC.PER_WINDOW
    assert c11["jobs"] == len(regs) and {k: c11[k] for k in same} == {k: c1[k] for k in same}


def test_mixed_list_plans_the_sum_of_its_single_size_plans(modsx):
    """direct and smoothed regions and two window sizes in one chunk: the tables of the second size lie behind the first's and the
    arena offsets run on behind direct jobs, which take no arena"""
    parts = [DC.regions_of(0, (3,)), DC.regions_of(47, (1,)), DC.regions_of(0, (0, 4)), DC.regions_of(985, (0, 3)), DC.regions_of(47, (2,)),
             DC.regions_of(0, (2,))]
    c, cuts = _plan(modsx, np.concatenate(parts))
    assert (c["calls"], c["chunks"]) == (1, 1) and not cuts, c
    singles = [_plan(modsx, p)[0] for p in parts]
    for k in ("jobs", "direct_jobs") + DC.PER_WINDOW:
        assert c[k] == sum(s[k] for s in singles), (k, c, singles)
    assert (c["jobs"], c["direct_jobs"], c["clamped_windows"]) == (8, 4, 2) and c["sample_tiles"] > 0, c
    # the same regions as two images
    c2, _ = _plan(modsx, [np.concatenate(parts[:3]), np.concatenate(parts[3:])])
    assert c2 == c
