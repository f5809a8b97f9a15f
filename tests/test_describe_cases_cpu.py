"""CPU: the inputs of the describe-path and describe-chunk GPU tests (tests/describe_cases.py) are fit for purpose, proven on the
oracle alone.

Measured (8 oracle threads, one region per task, the large windows first): the oracle over the whole sweep -- 122 window sizes and
the direct branch, three regions each -- takes 5.3 to 5.9 s of wall time, which P = 2329 and P = 2083 dominate; the views case
takes 1.5 s and the crafted image 4.3 s.  The module asserts that the sweep stays under SWEEP_CEILING_S = 60 s; it is shared by the
tests of this module through describe_cases.references().
"""
import time

import numpy as np
import pytest

from tests import describe_cases as DC

SWEEP_CEILING_S = 60.0


@pytest.fixture(scope="module")
def refs():
    t0 = time.time()
    r = DC.references()
    wall = time.time() - t0
    print("oracle over the sweep: %.1f s" % wall)
    # the GPU modules pay this once per run: past a minute, thin the sizes above 137 (never a boundary pair)
    assert wall < SWEEP_CEILING_S, "the oracle took %.1f s over the sweep: thin the sizes above 137 in tests/describe_cases.py, never a boundary pair" % wall
    return r


def test_image_has_full_mantissas():
    img = DC.image()
    assert img.shape == (DC.ROWS, DC.COLS) and img.dtype == np.float32
    assert img.min() >= 0.0 and img.max() <= 255.0
    not_eighths = np.mean(img * 8.0 != np.floor(img * 8.0))
    print("pixels that are no multiple of 1/8: %.4f" % not_eighths)
    assert not_eighths > 0.5


def test_sizes_hold_the_dense_range_and_both_sides_of_every_boundary():
    assert all(p % 2 == 1 for p in DC.SIZES) and list(DC.SIZES) == sorted(set(DC.SIZES))
    assert set(range(19, 137, 2)) <= set(DC.SIZES)
    for lo, hi in ((33, 35), (43, 45), (65, 67), (471, 473), (983, 985), (1023, 1025), (2329, DC.REFUSED_P)):
        assert lo in DC.SIZES and hi in DC.SIZES + (DC.REFUSED_P,), (lo, hi)
    for P in DC.SIZES + (DC.REFUSED_P,):
        assert DC.window_of(DC.s_of(P)) == P                     # s = (P - 3) / 2 at mr_size = 1 picks P exactly
    assert DC.window_of(DC.DIRECT_S) == 0 and DC.window_of(DC.DIRECT_S + 1.0) == 19      # the 0.4 edge: 15 / 41 and 17 / 41


def test_interior_windows_lie_inside_and_border_windows_do_not(oracle):
    for P in DC.SIZES:
        for x, y in DC.interior_corners(P):
            # interpolate()'s own no-border condition, which is inside [1, cols - 2] x [1, rows - 2]
            assert np.floor(x) >= 1 and np.ceil(x) <= DC.COLS - 3 and np.floor(y) >= 1 and np.ceil(y) <= DC.ROWS - 3, (P, x, y)
        r = DC.regions_of(P)
        k = r["det_kp"]
        for i, outside in enumerate((False, True, True)):
            # the oracle's own sampling of the P x P window: does it meet a pixel outside the image; how much of it does
            win, touched = oracle.interpolate(DC.image(), k["x"][i], k["y"][i], k["a11"][i], k["a12"][i], k["a21"][i], k["a22"][i], P, P)
            assert touched == outside, (P, i)
            if outside:
                assert np.mean(win == 0) > 0.5, (P, i)
        for f in ("x", "y", "a11", "a12", "a21", "a22", "s"):
            assert np.array_equal(r["det_kp"][f], r["reproj_kp"][f])


def test_reference_descriptors_are_distinct_and_fill_both_halves(refs):
    assert sorted(refs) == [0] + list(DC.SIZES)
    allv = np.concatenate([refs[P] for P in sorted(refs)])
    assert allv.shape == (3 * (len(DC.SIZES) + 1), 128)
    assert len({v.tobytes() for v in allv}) == len(allv), "two regions of the sweep have the same reference descriptor"
    assert (allv[:, :64] != 0).any(1).all() and (allv[:, 64:] != 0).any(1).all()


def test_chunk_cases_cut_where_the_gpu_test_needs_them(oracle, small_pair):
    a = small_pair[0]
    assert a.shape == (DC.ROWS, DC.COLS)
    regs, _ = DC.views_case(oracle, a)
    windows = [DC.window_of(s, DC.VIEWS_DESC_MR) for s in regs["det_kp"]["s"]]
    cuts = DC.greedy_cuts(windows)
    # the regions of a view: the identity carries img_id 0, view v > 0 carries v
    starts = [0] + [i for i in range(1, len(regs)) if regs["img_id"][i] != regs["img_id"][i - 1]]
    assert len(starts) == 11
    mid = [c for c in cuts if c not in starts]
    print("views: %d regions, %d floats of windows, cuts %r, views begin at %r" % (len(regs), sum(w * w for w in windows), cuts, starts))
    # if the 11 views go through one launch set: 5 chunks, cuts inside views; one of them inside a view other than the first
    assert len(cuts) >= 4 and len(mid) >= 3 and any(c > starts[1] for c in cuts)
    whole = [v for v in range(10) if not any(starts[v] <= c < starts[v + 1] for c in cuts) and not any(c == starts[v] for c in cuts)]
    assert whole, "no view lies whole inside a chunk"
    cw = [DC.window_of(s) for s in DC.crafted_regions()["det_kp"]["s"]]
    assert cw == [P for P, n in DC.CRAFTED_RUNS for _ in range(n)]
    assert 2083 * 2083 > DC.ARENA_FLOOR_FLOATS
    # 42 windows of 315 x 315 fill the arena; the P = 2083 window opens a chunk of its own windows (the empty-chunk guard) and the
    # direct-branch regions behind it, which need no arena, stay with it; the next P = 315 window closes that chunk
    assert DC.greedy_cuts(cw) == [42, 60, 81, 123]
