"""GPU: the certain-drop filter in front of the orientation launch changes no result.

Views: image A of the headline pair (1024x768, 5500 blobs, seed 12345; u8 in, f32 on the device) under the identity, tilt 2 at
phi 60 degrees and tilt 4 at phi 30 degrees through the views API against oracle.detect_describe_views -- regions field by
field, descriptors byte by byte -- with the orientation counters: some regions were left out, and launched + skipped is the
number of regions that pass DetectOrientation's own view-border test.
Filter off: the same calls in ONE child process with MODSX_ORI_PREFILTER=0 (tests/orient_prefilter_child.py; the switch is read
once per process) return the same bytes, skip nothing and launch what the filtered run launched + skipped.
Single-view path: match_pairs on the small pair, in process and in that child (the identity reprojection can skip nothing).
Public API: Context.detect_orientation is unfiltered.

Fault latch: a child that ends by a signal, with status 134 / 139, by the time limit, or with a failure whose stderr carries a HIP
error sets _FAULT; every later test of this module then fails at once -- no further process, no further use of the context."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import same_records
from tests import orient_prefilter_child as OC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "orient_prefilter_child.py")
# Time limit of the child: import, context creation and five launch sets -- about a second of work; the floor of 120 s that
# tests/test_gpu_match_shapes.py derives for such a child applies (import, context creation and a shared GPU vary by that much).
CHILD_TIMEOUT_S = 120
HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "device-side assert",
                   "unspecified launch failure", "queue error")
_FAULT = None


def _latch():
    if _FAULT is not None:
        pytest.fail("the switched-off child %s; nothing more is started on the GPU.  Its stderr ended:\n%s" % _FAULT, pytrace=False)


@pytest.fixture(scope="module")
def image_a():
    from mods_amd import synthetic
    a = synthetic.make_pair(768, 1024, 5500, 12345)[0]
    u8 = a.astype(np.uint8)
    u8.setflags(write=False)
    return u8


@pytest.fixture(scope="module")
def ref(oracle, image_a):
    """the oracle on the three views, computed once: the whole result, and per view the view image, its regions before
    orientation, and how many of them pass DetectOrientation's view-border test (maxAngNum = 0 with addUpRight returns exactly
    those), how many oriented regions there are and how many of those ReprojectRegions keeps"""
    gray = image_a.astype(np.float32)
    views = [oracle.make_view(t, p) for t, p in OC.VIEWS]
    regs, desc = oracle.detect_describe_views(gray, views, threads=len(views))
    per = []
    for vi, v in enumerate(views):
        img, Hm, ident = oracle.synth_view(gray, v)
        k = oracle.detect_hessaff(img, oracle.default_params(), tilt=1.0 if ident else abs(v.tilt), zoom=1.0 if ident else v.zoom)
        r0 = oracle.detect_affine_regions(k, img_id=0 if ident else vi)
        passing = len(oracle.detect_orientation(img, r0, max_ang=0, upright=1))
        ro = oracle.detect_orientation(img, r0, half=0, max_ang=1, th=0.8)
        kept = len(oracle.reproject_regions(ro, Hm.reshape(9), gray.shape[1], gray.shape[0]))
        per.append(dict(img=img, r0=r0, passing=passing, oriented=len(ro), kept=kept))
    assert sum(p["kept"] for p in per) == len(regs)
    for a in (regs, desc):
        a.setflags(write=False)
    return dict(regs=regs, desc=desc, per=per)


@pytest.fixture(scope="module")
def filtered(ctx, modsx, image_a, small_pair):
    """run_all in this process: filter on"""
    assert os.environ.get("MODSX_ORI_PREFILTER", "1") != "0", "this module is about the filter being on in the parent"
    return OC.run_all(modsx, ctx, image_a, small_pair[0], small_pair[1])


@pytest.fixture(scope="module")
def unfiltered(image_a, small_pair, tmp_path_factory):
    """run_all in a child with MODSX_ORI_PREFILTER=0"""
    global _FAULT
    _latch()
    d = str(tmp_path_factory.mktemp("orient_prefilter"))
    inp, outp = os.path.join(d, "in.npz"), os.path.join(d, "out.npz")
    np.savez(inp, image_u8=image_a, small_a=small_pair[0], small_b=small_pair[1])
    env = dict(os.environ, MODSX_ORI_PREFILTER="0")
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
    assert p.returncode == 0, "the switched-off child failed with status %d:\n%s" % (p.returncode, err)
    return dict(np.load(outp))


def test_views_equal_oracle_and_some_regions_are_skipped(filtered, ref, modsx):
    _latch()
    per = ref["per"]
    print("oracle per view (passing, oriented, kept):", [(p["passing"], p["oriented"], p["kept"]) for p in per])
    launched, skipped = (int(v) for v in filtered["views_counts"])
    print("orientation jobs launched %d, skipped %d" % (launched, skipped))
    assert len(ref["regs"]) > 3000 and all(p["kept"] < p["oriented"] for p in per[1:])      # reprojection drops regions of the tilted views
    assert same_records(filtered["views_regs"], ref["regs"].view(modsx.REGION))
    assert filtered["views_desc"].dtype == ref["desc"].dtype and filtered["views_desc"].tobytes() == ref["desc"].tobytes()
    assert list(filtered["views_per_view"]) == [p["kept"] for p in per]
    assert skipped > 0
    assert launched + skipped == sum(p["passing"] for p in per)
    # nothing that survives was skipped (maxAngNum = 1: at most one oriented region per job)
    assert launched >= sum(p["kept"] for p in per)


def test_filter_off_gives_the_same_bytes(filtered, unfiltered, modsx):
    _latch()
    assert same_records(unfiltered["views_regs"].view(modsx.REGION), filtered["views_regs"])
    assert unfiltered["views_desc"].tobytes() == filtered["views_desc"].tobytes()
    assert np.array_equal(unfiltered["views_per_view"], filtered["views_per_view"])
    launched, skipped = (int(v) for v in filtered["views_counts"])
    assert int(unfiltered["views_counts"][1]) == 0
    assert int(unfiltered["views_counts"][0]) == launched + skipped


def test_single_view_pairs_equal_with_filter_off(filtered, unfiltered, modsx):
    _latch()
    assert filtered["pair_regions"].min() > 100 and len(filtered["pair_tentatives"]) > 20
    for f in ("regions", "scalars", "ransac_inlier", "verified", "H"):
        assert np.array_equal(unfiltered["pair_" + f], filtered["pair_" + f]), f
    g, s = unfiltered["pair_tentatives"], filtered["pair_tentatives"]
    assert len(g) == len(s)
    for f in s.dtype.names:
        assert np.array_equal(g[f], s[f]), f
    launched, skipped = (int(v) for v in filtered["pair_counts"])
    print("single-view pair: orientation jobs launched %d, skipped %d" % (launched, skipped))
    # the identity onto the image's own size repeats the view-border test on the rotated shape: what passed that test unrotated
    # has |a11| + |a12| >= the row norm inside the bounds, so nothing is certain before the angle is known
    assert launched > 200 and skipped == 0
    assert tuple(int(v) for v in unfiltered["pair_counts"]) == (launched, 0)


def test_public_detect_orientation_is_unfiltered(ctx, modsx, oracle, ref):
    _latch()
    p = ref["per"][1]                                        # tilt 2: a view whose reprojection drops a fifth of the oriented regions
    want = oracle.detect_orientation(p["img"], p["r0"], half=0, max_ang=1, th=0.8)
    assert len(want) == p["oriented"] > p["kept"]
    im = ctx.upload(p["img"])
    modsx.orientation_counts(reset=True)
    got = ctx.detect_orientation(im, p["r0"].view(modsx.REGION), half=0, max_ang=1, th=0.8)
    counts = modsx.orientation_counts(reset=True)
    im.free()
    assert len(got) == len(want) and same_records(got, want.view(modsx.REGION))
    assert counts == (p["passing"], 0)
