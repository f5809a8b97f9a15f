"""The slim form of k_describe (one LDS buffer per region) and its redo launch, bit for bit.

Every region of tests/describe_slim_cases.py takes the grid branch (fast = 0, ceil(s * mr_size) = 10) unless a case says
otherwise.  The descriptors are compared with oracle.describe_patch on the oracle's own patch of the region (the Half types
with dspsift_model's f64 norms of its histogram); which workgroups the redo launch runs again is predicted on the CPU from
sift_gather_model.decide on the oracle's normalised patch and the pairing rule of sift_patch_cases.workgroups, and
Context.describe_slim_counters / describe_counters confirm it.  The raw-histogram and patch-out forms keep the full kernel
(they are not slim launches): one case shows that they leave the slim counters alone and still match.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import describe_slim_cases as DS
import sift_patch_cases as SC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def handle(ctx):
    h = ctx.upload(DS.image())
    yield h
    h.free()


def counters(ctx):
    c = dict(ctx.describe_slim_counters())
    c["ordered_workgroups"] = ctx.describe_counters()["ordered_workgroups"]
    return c


def run(ctx, modsx, handle, cen, pn, dt, scales=None):
    regs = DS.regions(modsx.REGION, cen) if scales is None else np.concatenate(
        [DS.regions(modsx.REGION, [c], s) for c, s in zip(cen, scales)])
    c0 = counters(ctx)
    got = ctx.describe_regions(handle, regs, mr_size=DS.MR_SIZE, fast=DS.FAST, photo_norm=pn, desc_type=dt)
    c1 = counters(ctx)
    return got, {k: c1[k] - c0[k] for k in c0}


def check_rows(oracle, modsx, got, cen, pn, dt):
    for q, c in enumerate(cen):
        assert np.array_equal(got[q], DS.reference(oracle, modsx, c, pn)["desc"][dt]), (q, c, pn, dt)


def expect_slim(delta, redo):
    assert delta["slim_launches"] == 1 and delta["full_launches"] == 0, delta
    assert delta["redo_workgroups"] == redo and delta["ordered_workgroups"] == redo, (delta, redo)


def test_textured_regions_are_order_free_on_the_cpu(oracle, modsx):
    """the premise of the cases below, and the oracle's two routes agree: describe_patch on extract_patch == describe_regions"""
    for pn in (0, 1):
        assert not DS.inexact(oracle, modsx, DS.TEX, pn).any()
        assert DS.inexact(oracle, modsx, DS.ZERO_L + DS.ZERO_R, pn).all()
        whole = oracle.describe_regions(DS.image(), DS.regions(modsx.REGION, DS.TEX), mr_size=DS.MR_SIZE, fast=DS.FAST,
                                        photo_norm=pn, rootsift=1)
        check_rows(oracle, modsx, whole, DS.TEX, pn, 1)


@pytest.mark.parametrize("pn", (0, 1))
@pytest.mark.parametrize("dt", (0, 1, 2, 3))
def test_order_free_even(ctx, modsx, oracle, handle, pn, dt):
    cen = DS.lists()["free_even"][0]
    got, d = run(ctx, modsx, handle, cen, pn, dt)
    expect_slim(d, 0)
    check_rows(oracle, modsx, got, cen, pn, dt)


@pytest.mark.parametrize("pn", (0, 1))
def test_odd_count(ctx, modsx, oracle, handle, pn):
    cen = DS.lists()["free_odd"][0]
    got, d = run(ctx, modsx, handle, cen, pn, 1)
    expect_slim(d, 0)
    check_rows(oracle, modsx, got, cen, pn, 1)


@pytest.mark.parametrize("name", ("forced_slot1", "forced_slot0"))
@pytest.mark.parametrize("pn", (0, 1))
def test_forced_redo(ctx, modsx, oracle, handle, name, pn):
    cen = DS.lists()[name][0]
    want = SC.predicted_ordered(cen, DS.inexact(oracle, modsx, cen, pn))
    assert want == (1 if name == "forced_slot1" else 2)
    got, d = run(ctx, modsx, handle, cen, pn, 1)
    expect_slim(d, want)
    check_rows(oracle, modsx, got, cen, pn, 1)
    # the textured region beside the zero region: its descriptor from the order-free call
    free, _ = run(ctx, modsx, handle, DS.TEX[:4], pn, 1)
    assert np.array_equal(got[cen.index(DS.TEX[0])], free[0])


def test_redo_list_longer_than_the_redo_grid(ctx, modsx, oracle, handle):
    cen = DS.lists()["long_redo"][0]
    want = SC.predicted_ordered(cen, DS.inexact(oracle, modsx, cen, 1))
    assert want > 64 and len(cen) == 142
    got, d = run(ctx, modsx, handle, cen, 1, 1)
    expect_slim(d, want)
    check_rows(oracle, modsx, got, cen, 1, 1)


def test_empty_then_listed_then_empty(ctx, modsx, oracle, handle):
    """the list's count word is reset between launch sets, in both directions"""
    L = DS.lists()
    for name, redo in (("free_even", 0), ("forced_slot0", 2), ("free_even", 0), ("forced_slot1", 1), ("free_odd", 0)):
        cen = L[name][0]
        got, d = run(ctx, modsx, handle, cen, 1, 1)
        expect_slim(d, redo)
        check_rows(oracle, modsx, got, cen, 1, 1)


def test_direct_region_keeps_the_full_kernel(ctx, modsx, oracle, handle):
    cen, scales = DS.lists()["mixed_direct"]
    got, d = run(ctx, modsx, handle, cen, 1, 1, scales)
    assert d["full_launches"] == 1 and d["slim_launches"] == 0 and d["redo_workgroups"] == 0, d
    check_rows(oracle, modsx, got[:4], cen[:4], 1, 1)
    regs = np.concatenate([DS.regions(modsx.REGION, [c], s) for c, s in zip(cen, scales)])
    want = oracle.describe_regions(DS.image(), regs, mr_size=DS.MR_SIZE, fast=DS.FAST, photo_norm=1, rootsift=1)
    assert np.array_equal(got, want)
    slim, d = run(ctx, modsx, handle, cen[:4], 1, 1)
    expect_slim(d, 0)
    assert np.array_equal(slim, got[:4])


def test_raw_and_patch_forms_keep_the_full_kernel(ctx, modsx, oracle, handle):
    cen = DS.lists()["forced_slot1"][0]
    regs = DS.regions(modsx.REGION, cen)
    c0 = counters(ctx)
    raw = ctx.describe_regions_raw(handle, regs, mr_size=DS.MR_SIZE, fast=DS.FAST, photo_norm=1)
    patches = ctx.extract_patches(handle, regs, mr_size=DS.MR_SIZE, fast=DS.FAST, photo_norm=1)
    c1 = counters(ctx)
    assert all(c1[k] == c0[k] for k in ("slim_launches", "full_launches", "redo_workgroups")), (c0, c1)
    for q, c in enumerate(cen):
        ref = DS.reference(oracle, modsx, c, 1)
        assert np.array_equal(raw[q], ref["raw"], equal_nan=True), (q, c)
        assert np.array_equal(patches[q], ref["patch"], equal_nan=True), (q, c)


@pytest.fixture(scope="module")
def full_kernel_child(tmp_path_factory):
    """the same lists and the two-class pair in a fresh process with MODSX_DESCRIBE_SLIM=0"""
    outp = str(tmp_path_factory.mktemp("slim") / "child.npz")
    env = dict(os.environ, MODSX_DESCRIBE_SLIM="0")
    subprocess.run([sys.executable, os.path.join(HERE, "describe_slim_cases.py"), outp], check=True, env=env, timeout=300)
    z = np.load(outp)
    return {k: z[k] for k in z.files}


def test_slim_off_in_a_child_is_byte_identical(ctx, modsx, handle, full_kernel_child):
    child = full_kernel_child
    assert child["slim_counters"][0] == 0 and child["slim_counters"][2] == 0 and child["slim_counters"][1] > 0
    c0 = counters(ctx)
    here = DS.describe_all(modsx, ctx, handle)
    c1 = counters(ctx)
    assert c1["slim_launches"] - c0["slim_launches"] == len(here) - 1      # every list but the one with a direct region
    for name, got in here.items():
        assert got.tobytes() == child[name].tobytes(), name


def test_two_classes_in_one_step(ctx, modsx, small_pair, full_kernel_child):
    """RootSIFT + HalfRootSIFT from one histogram (nOut = 2) through slim + redo: the pair's result equals the full kernel's"""
    c0 = counters(ctx)
    here = DS.pair_result(modsx, ctx, small_pair)
    c1 = counters(ctx)
    d = {k: c1[k] - c0[k] for k in c0}
    print("two classes:", d)
    assert d["slim_launches"] > 0 and d["full_launches"] == 0, d
    assert d["redo_workgroups"] == d["ordered_workgroups"] > 0, d
    for k, v in here.items():
        assert np.array_equal(v, full_kernel_child[k], equal_nan=True), k
