"""GPU: describe_batch cut into chunks -- the cut, the continuation in the middle of an image's region list, outIdx across chunks
and images, the alternating staging blob, the second descriptor class's buffers -- gives the bytes of the single-chunk run and
of the oracle.

The window arena is 192 MiB by default and every other describe call of the suite fits it many times over: one chunk.
MODSX_ARENA_MB is read once per process, so ONE child (tests/describe_chunk_child.py) runs the cases at MODSX_ARENA_MB=16, the
floor (4 194 304 floats); the parent runs the same run_all in process at the default arena.  Cases (tests/describe_cases.py; the
cuts the planner itself -- mods_amd/csrc/describe_plan.cpp through mods_amd.describe_plan -- gives for them are proven on the CPU
in tests/test_describe_plan_cpu.py, and here the counters of the views and the crafted device calls must equal that plan's):
  views    image 0 of the small pair under TiltSet 1, 2, 4, 6, 8 (11 views) with desc_mrSize = 24: against
           oracle.detect_describe_views, regions field by field, descriptors byte by byte
  crafted  60 regions of P = 315, one of P = 2083 (larger than the arena: the `&& count` guard lets it open a chunk of its own
           windows), 20 direct-branch regions, 60 of P = 315 through describe_regions: against oracle.describe_regions
  pair     match_pair with RootSIFT + HalfRootSIFT and desc_mrSize = 24: child against parent, field by field
What the counters of the child must show: at least 4 chunks in one call (both staging blobs are reused), at least 3 chunks that
began in the middle of an image's region list, at least 1 that began at a later image; in the parent every call is one chunk.

Fault latch: a child that ends by a signal, with status 134 / 139, by the time limit, or with a failure whose stderr carries a HIP
error sets _FAULT; every later test of this module then fails at once -- no further process, no further use of the context."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import same_records
from tests import describe_cases as DC
from tests import describe_chunk_child as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "describe_chunk_child.py")
# Time limit of the child: import, context creation and three cases -- about a second of work; the floor of 120 s that
# tests/test_gpu_match_shapes.py derives for such a child applies (import, context creation and a shared GPU vary by that much).
CHILD_TIMEOUT_S = 120
HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "device-side assert",
                   "unspecified launch failure", "queue error")
_FAULT = None


def _latch():
    if _FAULT is not None:
        pytest.fail("the small-arena child %s; nothing more is started on the GPU.  Its stderr ended:\n%s" % _FAULT, pytrace=False)


def _cnt(modsx, arr):
    return dict(zip(modsx.DESCRIBE_COUNTERS, (int(v) for v in arr)))


@pytest.fixture(scope="module")
def ref(oracle, small_pair):
    """the oracle on the views case and on the crafted image, computed once"""
    regs, desc = DC.views_case(oracle, small_pair[0])
    crafted = oracle.describe_regions(DC.image(), DC.crafted_regions(), mr_size=DC.MR_SIZE)
    crafted.setflags(write=False)
    return dict(views_regs=regs, views_desc=desc, crafted=crafted)


@pytest.fixture(scope="module")
def one_chunk(ctx, modsx, small_pair):
    """run_all in this process: the default arena"""
    assert not os.environ.get("MODSX_ARENA_MB"), "this module is about the default arena in the parent"
    return CC.run_all(modsx, ctx, small_pair[0], small_pair[1])


@pytest.fixture(scope="module")
def chunked(small_pair, tmp_path_factory):
    """run_all in a child with MODSX_ARENA_MB=16"""
    global _FAULT
    _latch()
    d = str(tmp_path_factory.mktemp("describe_chunks"))
    inp, outp = os.path.join(d, "in.npz"), os.path.join(d, "out.npz")
    np.savez(inp, small_a=small_pair[0], small_b=small_pair[1])
    env = dict(os.environ, MODSX_ARENA_MB="16")
    try:
        p = subprocess.run([sys.executable, CHILD, inp, outp], env=env, timeout=CHILD_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except subprocess.TimeoutExpired as e:
        _FAULT = ("did not end within %d s" % CHILD_TIMEOUT_S, (e.stderr or b"").decode(errors="replace")[-1500:])
        _latch()
    err = p.stderr.decode(errors="replace")[-1500:]
    whole = p.stderr.decode(errors="replace").lower()
    if p.returncode < 0 or p.returncode in (134, 139) or (p.returncode != 0 and any(m in whole for m in HIP_ERROR_MARKS)):
        _FAULT = ("ended with status %d" % p.returncode, err)
        _latch()
    assert p.returncode == 0, "the small-arena child failed with status %d:\n%s" % (p.returncode, err)
    return dict(np.load(outp))


def _booked_equals_plan(modsx, got, case):
    """what the device call booked is what the planner alone gives for its regions at the same arena (max_chunks is a running
    maximum of the context: at least the plan's)"""
    c, p = _cnt(modsx, got[case + "_counters"]), _cnt(modsx, got[case + "_plan"])
    assert {k: c[k] for k in DC.SUMMED} == {k: p[k] for k in DC.SUMMED}, (case, c, p)
    assert c["max_chunks"] >= p["max_chunks"] == p["chunks"], (case, c, p)


def _views_equal_oracle(got, ref, modsx):
    assert len(ref["views_regs"]) > 400
    assert same_records(got["views_regs"].view(modsx.REGION), ref["views_regs"].view(modsx.REGION))
    assert got["views_desc"].dtype == ref["views_desc"].dtype and np.array_equal(got["views_desc"], ref["views_desc"])
    assert int(got["views_per_view"].sum()) == len(ref["views_regs"]) and len(got["views_per_view"]) == 11


def test_one_chunk_views_and_crafted_equal_oracle(one_chunk, ref, modsx):
    _latch()
    _views_equal_oracle(one_chunk, ref, modsx)
    assert np.array_equal(one_chunk["crafted_desc"], ref["crafted"])
    for case in ("views", "crafted", "pair"):
        c = _cnt(modsx, one_chunk[case + "_counters"])
        print("default arena, %s: %r" % (case, c))
        assert c["calls"] >= 1 and c["chunks"] == c["calls"], "%s: every call must be exactly one chunk at the default arena: %r" % (case, c)
        assert c["chunks_mid_image"] == 0 and c["chunks_later_image"] == 0, (case, c)
    for case in ("views", "crafted"):
        _booked_equals_plan(modsx, one_chunk, case)
    assert _cnt(modsx, one_chunk["crafted_counters"])["jobs"] == len(DC.crafted_regions())
    assert _cnt(modsx, one_chunk["views_counters"])["jobs"] == len(ref["views_regs"])


def test_chunked_views_equal_oracle(chunked, ref, modsx):
    _latch()
    c = _cnt(modsx, chunked["views_counters"])
    print("16 MiB arena, views: %r; regions per view %r" % (c, list(chunked["views_per_view"])))
    _views_equal_oracle(chunked, ref, modsx)
    assert c["jobs"] == len(ref["views_regs"])
    assert c["chunks"] > c["calls"] and c["chunks_mid_image"] >= 1 and c["chunks_later_image"] >= 1, c
    _booked_equals_plan(modsx, chunked, "views")


def test_chunked_crafted_image_equals_oracle(chunked, ref, modsx):
    _latch()
    c = _cnt(modsx, chunked["crafted_counters"])
    print("16 MiB arena, crafted: %r" % (c,))
    assert np.array_equal(chunked["crafted_desc"], ref["crafted"])
    windows = [DC.window_of(s) for s in DC.crafted_regions()["det_kp"]["s"]]
    # one call of one image: every chunk after the first begins in the middle of the list, none at a later image
    assert (c["calls"], c["chunks"], c["chunks_mid_image"], c["chunks_later_image"]) == (1, len(DC.greedy_cuts(windows)) + 1, len(DC.greedy_cuts(windows)), 0), c
    assert c["jobs"] == len(windows) and c["direct_jobs"] == windows.count(0)
    _booked_equals_plan(modsx, chunked, "crafted")
    assert c["sample_tiles"] == ((2083 + 63) // 64) * ((2083 + 127) // 128), "the P = 2083 window goes through k_patch_sample: %r" % (c,)


def test_chunked_two_class_pair_equals_one_chunk_run(chunked, one_chunk, modsx):
    _latch()
    c = _cnt(modsx, chunked["pair_counters"])
    print("16 MiB arena, pair: %r; regions %r, %d unique tentatives" % (c, tuple(one_chunk["pair_regions"]), len(one_chunk["pair_tentatives"])))
    assert one_chunk["pair_regions"].min() > 50 and len(one_chunk["pair_tentatives"]) > 20
    for f in ("regions", "scalars", "ransac_inlier", "verified", "H"):
        assert np.array_equal(chunked["pair_" + f], one_chunk["pair_" + f]), f
    g, s = chunked["pair_tentatives"], one_chunk["pair_tentatives"]
    assert len(g) == len(s)
    for f in s.dtype.names:
        assert np.array_equal(g[f], s[f]), f
    assert c["chunks"] > c["calls"], "the two-class pair did not cross a chunk boundary: %r" % (c,)


def test_child_counters_show_the_chunking(chunked, modsx):
    _latch()
    cs = [_cnt(modsx, chunked[k + "_counters"]) for k in ("views", "crafted", "pair")]
    assert max(c["max_chunks"] for c in cs) >= 4, "no call of the child ran 4 chunks (both staging blobs reused): %r" % (cs,)
    assert sum(c["chunks_mid_image"] for c in cs) >= 3, cs
    assert sum(c["chunks_later_image"] for c in cs) >= 1, cs
