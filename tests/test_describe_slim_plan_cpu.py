"""DescChunkPlan::slim on the host alone (modsx_debug_describe_plan_slim): a chunk may take the slim form of the describe kernel
exactly when it holds no region of the direct branch (P == 0)."""
import numpy as np

import sift_patch_cases as SC

MR = 10.0
GRID_S, DIRECT_S = 1.0, 0.3          # ceil(10) = 10: a 21-pixel window, P = 23; ceil(3) = 3: 7 / 41 <= 0.4, the direct branch
P_GRID = 23


def regs(modsx, scales):
    return np.concatenate([SC.regions(modsx.REGION, [(100 + 3 * q, 100)], s) for q, s in enumerate(scales)])


def plan(modsx, scales, **kw):
    r = regs(modsx, scales)
    p = modsx.describe_plan(r, MR, **kw)
    assert p["rc"] == 0
    slim = modsx.describe_plan_slim(r, MR, **kw)
    assert len(slim) == p["counters"]["chunks"]
    return p, slim


def test_mixed_chunk(modsx):
    p, slim = plan(modsx, [GRID_S, DIRECT_S, GRID_S])
    assert p["counters"]["direct_jobs"] == 1 and slim == [False]
    assert plan(modsx, [GRID_S, GRID_S, DIRECT_S])[1] == [False] and plan(modsx, [DIRECT_S, GRID_S])[1] == [False]


def test_all_grid_chunk(modsx):
    p, slim = plan(modsx, [GRID_S] * 5)
    assert p["counters"]["direct_jobs"] == 0 and p["counters"]["jobs"] == 5 and slim == [True]
    assert plan(modsx, [GRID_S])[1] == [True]


def test_all_direct_chunk(modsx):
    p, slim = plan(modsx, [DIRECT_S] * 4)
    assert p["counters"]["direct_jobs"] == 4 and slim == [False]


def test_fast_extraction_is_all_direct(modsx):
    p, slim = plan(modsx, [GRID_S] * 4, fast=1)
    assert p["counters"]["direct_jobs"] == 4 and slim == [False]


def test_two_chunks_one_with_a_direct_job(modsx):
    arena = 3 * P_GRID * P_GRID                       # three grid windows fill a chunk; a direct region takes no arena
    p, slim = plan(modsx, [GRID_S] * 3 + [GRID_S, GRID_S, DIRECT_S], arena_floats=arena)
    assert p["cuts"] == [3] and slim == [True, False]
    p, slim = plan(modsx, [GRID_S, DIRECT_S, GRID_S] + [GRID_S] * 3, arena_floats=arena)
    assert p["cuts"] == [4] and slim == [False, True]
    p, slim = plan(modsx, [GRID_S] * 7, arena_floats=arena)
    assert p["cuts"] == [3, 6] and slim == [True, True, True]


def test_empty_call_has_no_chunk(modsx):
    assert modsx.describe_plan_slim(np.zeros(0, modsx.REGION), MR) == []
