"""SIFT histogram parity per patch: the planted patches of tests/sift_patch_cases.py through both gathers of k_describe.

Every case runs under its options through Context.describe_regions (against oracle.describe_patch; the Half types against
dspsift_model's f64 norms of its histogram), Context.describe_regions_raw (against dspsift_model.raw) and Context.extract_patches
(against the planted or the oracle's normalised patch), bit for bit, in three arrangements:
  1  with the cases that need the same gather: the order-free ones in one call, which must add nothing to `ordered_workgroups`, and
     the ones the model sends to the ordered gather alone, one call each (one call for all of them where an image has more
     than 16), where every workgroup must count;
  2  every case followed by the blank cell to its right: case in slot 0 of its workgroup, a region of zeros in slot 1 -- the
     workgroup takes the ordered gather, the counter must say so and the case's three outputs must not change;
  3  the blank cell to its left first: the case in slot 1.
The counter's difference over a call is compared with what sift_patch_cases.predicted_ordered gives for the call's list, from the
model's decision per region (tests/sift_gather_model.py) and the launch rule; tests/test_sift_patch_cases_cpu.py proves both on the
CPU.  With MODSX_TEST_ORDERED_ONLY=1 (a library built with -DMODSX_DESC_ORDERED_ONLY, where every workgroup takes the ordered
gather) the expected difference is the number of workgroups instead.
"""
import os

import numpy as np
import pytest

import sift_patch_cases as SC

pytestmark = pytest.mark.gpu
F = np.float32
ORDERED_ONLY = os.environ.get("MODSX_TEST_ORDERED_ONLY", "") == "1"


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def ordered_delta(ctx, fn):
    c0 = ctx.describe_counters()["ordered_workgroups"]
    out = fn()
    return out, ctx.describe_counters()["ordered_workgroups"] - c0


def expected_ordered(centres, inexact):
    return (len(centres) + 1) // 2 if ORDERED_ONLY else SC.predicted_ordered(centres, inexact)


def run_list(ctx, modsx, oracle, handle, centres, rows, cases, pn, desc_types, inexact, want=None, raw=True, patches=True):
    """one region list through the three entries; rows[q] = position of case cases[q] in the list (every other position is a blank
    cell), inexact: per list position.  Returns the case rows of every output."""
    regs = SC.regions(modsx.REGION, centres)
    expect = expected_ordered(centres, inexact)
    if want is not None and not ORDERED_ONLY:
        assert expect == want, (expect, want)
    blank = np.setdiff1d(np.arange(len(centres)), rows)
    out = {}
    names = [SC.planted()[i]["name"] for i in cases]
    for dt in desc_types:
        got, delta = ordered_delta(ctx, lambda: ctx.describe_regions(handle, regs, mr_size=SC.MR_SIZE, fast=SC.FAST, photo_norm=pn, desc_type=dt))
        assert delta == expect, ("ordered_workgroups", delta, expect, pn, dt)
        assert not got[blank].any()
        for q, i in enumerate(cases):
            assert np.array_equal(got[rows[q]], SC.desc_of(oracle, i, pn, dt)), (names[q], pn, dt)
        out[dt] = got[rows]
    if raw:
        got, delta = ordered_delta(ctx, lambda: ctx.describe_regions_raw(handle, regs, mr_size=SC.MR_SIZE, fast=SC.FAST, photo_norm=pn))
        assert delta == expect, ("ordered_workgroups (raw)", delta, expect, pn)
        assert not got[blank].any()
        for q, i in enumerate(cases):
            if SC.raw_compared(SC.planted()[i]):
                assert same(got[rows[q]], SC.raw_of(oracle, i, pn)), (names[q], pn)
        out["raw"] = got[rows]
    if patches:
        got = ctx.extract_patches(handle, regs, mr_size=SC.MR_SIZE, fast=SC.FAST, photo_norm=pn)
        assert not got[blank].any()
        for q, i in enumerate(cases):
            assert same(got[rows[q]], SC.reference(oracle, i, pn)["patch"]), (names[q], pn)
        out["patches"] = got[rows]
    return out


@pytest.mark.parametrize("k,pn", SC.image_params())
def test_three_arrangements(ctx, modsx, oracle, k, pn):
    im = SC.images()[k]
    cases, cen, n = im["cases"], im["centres"], len(im["cases"])
    handle = ctx.upload(im["img"])
    try:
        dts = im["options"]["desc_types"]
        inexact = np.array([SC.inexact_of(oracle, i, pn) for i in cases])
        alone = {}
        free, need = np.nonzero(~inexact)[0], np.nonzero(inexact)[0]
        # the order-free cases in one call; the others one call each while they are few (a region alone is its own partner: its
        # trigger decides), in one call of their own otherwise
        lists = [(free, 0)] + ([(need[q:q + 1], 1) for q in range(len(need))] if len(need) <= 16 else [(need, (len(need) + 1) // 2)])
        for sel, want in lists:
            if len(sel):
                got = run_list(ctx, modsx, oracle, handle, cen[sel], np.arange(len(sel)), [cases[q] for q in sel], pn, dts,
                               inexact[sel], want=want)
                for key, rows in got.items():
                    alone.setdefault(key, np.zeros((n,) + rows.shape[1:], rows.dtype))[sel] = rows
        both = np.ones(2 * n, bool)                     # a blank cell in every workgroup: all of them ordered
        slot0 = run_list(ctx, modsx, oracle, handle, np.stack([cen, im["right"]], 1).reshape(-1, 2), np.arange(0, 2 * n, 2), cases, pn,
                         dts, both, want=n)
        slot1 = run_list(ctx, modsx, oracle, handle, np.stack([im["left"], cen], 1).reshape(-1, 2), np.arange(1, 2 * n, 2), cases, pn,
                         dts, both, want=n)
        for key in alone:                               # unchanged by the partner and by the slot, compared or not with a model
            assert same(alone[key], slot0[key]) and same(alone[key], slot1[key]), (im["group"], pn, key)
    finally:
        handle.free()


@pytest.mark.parametrize("group,pn", [("gather+magnitude", 0), ("random", 0), ("random", 1), ("photometric", 1)])
def test_call_sizes_and_mixed_calls(ctx, modsx, oracle, group, pn):
    """calls of 1, 2, 3, 64 and 65 regions and the whole list, trigger and ordinary regions mixed as they come: the counter adds the
    model's count of workgroups with at least one region that needs the ordered gather"""
    im = next(m for m in SC.images() if m["group"] == group)
    cases, cen, n = im["cases"], im["centres"], len(im["cases"])
    inexact = np.array([SC.inexact_of(oracle, i, pn) for i in cases])
    handle = ctx.upload(im["img"])
    try:
        for size in sorted({min(s, n) for s in (1, 2, 3, 64, 65, n)}):
            for first in sorted({0, n - size}):
                sel = np.arange(first, first + size)
                run_list(ctx, modsx, oracle, handle, cen[sel], np.arange(size), [cases[q] for q in sel], pn, (1,), inexact[sel],
                         raw=size <= 3 or size == n, patches=False)
        if group == "gather+magnitude":
            mixed = SC.predicted_ordered(cen, inexact)
            assert 0 < mixed < (n + 1) // 2                 # some workgroups of the whole list are ordered and some are not
    finally:
        handle.free()


def test_ramps_as_one_call(ctx, modsx, oracle):
    """every ramp (the whole oTab) in one call of about 2050 regions, cells side by side"""
    idx = [i for i, c in enumerate(SC.planted()) if c["family"] == "ramps"]
    img, cen = SC.compose_compact(np.stack([SC.planted()[i]["patch"] for i in idx]))
    inexact = np.array([SC.inexact_of(oracle, i, 0) for i in idx])
    assert not inexact.any()
    handle = ctx.upload(img)
    try:
        run_list(ctx, modsx, oracle, handle, cen, np.arange(len(idx)), idx, 0, (1,), inexact, want=0)
    finally:
        handle.free()
