"""MSER against the reference's OWN sources: detectors/mser compiled in place into oracle/_ref/libmser_ref.so
(oracle/Makefile, oracle/ref_mser_shim.cpp) and called through oracle.detect_msers_ref.  No GPU.

Every comparison is np.array_equal per field on the nine fields DetectMSERs sets (mser_ref_cases.FIELDS); there are no tolerances.
  * the product (modsx.detect_msers_u8, mods_amd/csrc/mser.cpp) == the reference, directly, on every case of tests/mser_ref_cases.py;
  * the restatement (oracle.detect_msers, oracle/oracle_mser.cpp) == the reference on the same cases and on the images the GPU suite
    compares the device paths on, which makes those comparisons pinned in turn;
  * trunc_u8_model == the reference's own (unsigned char)float;
  * the host pool (modsx_debug_msers_views_u8) == the reference view by view;
  * the reference repeats itself; the binding refuses what the reference faults on.
The reference keeps its state in file-level statics: it is called from the test thread only (the binding holds a lock besides).
Its answers are computed once per case (REF) and shared; nothing writes to them."""
import ctypes as C

import numpy as np
import pytest

import mser_front_cases as MC
import mser_ref_cases as RC
from common import need_mser_ref

GROUPS = RC.all_groups()
REF = {}          # case name -> the reference's records (read-only)


def _ref(oracle, case):
    name, img, kw = case
    if name not in REF:
        need_mser_ref(oracle)
        k, tilt, zoom = RC.split_kw(kw)
        r = oracle.detect_msers_ref(img, tilt=tilt, zoom=zoom, **k)
        r.setflags(write=False)
        REF[name] = r
    return REF[name]


def _same(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for f in RC.FIELDS:
        assert np.array_equal(got[f], ref[f]), (what, f)


def _u8(img):
    """the bytes DetectMSERs makes of the f32 pixels: exact for the integer-valued images, the x86 rule (pinned below) otherwise"""
    u8 = MC.trunc_u8_model(img)
    if np.isfinite(img).all() and img.min() >= 0 and img.max() <= 255 and np.array_equal(np.trunc(img), img):
        assert np.array_equal(u8, img.astype(np.uint8))
    return u8


def test_case_inventory():
    """at least 800 product-vs-reference cases, every image large enough for the reference, every name once"""
    names = [c[0] for g in GROUPS.values() for c in g]
    assert len(names) == len(set(names)) >= 800
    assert all(c[1].size >= RC.MIN_PIXELS and c[1].dtype == np.float32 for g in GROUPS.values() for c in g)
    assert len(RC.sweep_groups()) == len(RC.SWEEP_KINDS) * len(RC.SWEEP_SHAPES) and len(RC.SWEEP_PARAMS) == 12


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_product_equals_reference(modsx, oracle, group):
    for case in GROUPS[group]:
        name, img, kw = case
        k, tilt, zoom = RC.split_kw(kw)
        got = modsx.detect_msers_u8(_u8(img), modsx.default_mser_params(**k), tilt=tilt, zoom=zoom)
        _same(got, _ref(oracle, case), name)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_restatement_equals_reference(oracle, group):
    for case in GROUPS[group]:
        name, img, kw = case
        k, tilt, zoom = RC.split_kw(kw)
        _same(oracle.detect_msers(img, tilt=tilt, zoom=zoom, **k), _ref(oracle, case), name)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_reference_repeats_itself(oracle, group):
    for case in GROUPS[group]:
        name, img, kw = case
        k, tilt, zoom = RC.split_kw(kw)
        first = _ref(oracle, case)
        _same(oracle.detect_msers_ref(img, tilt=tilt, zoom=zoom, **k), first, name)


def test_restatement_equals_reference_on_the_gpu_suites_images(oracle):
    """tests/test_gpu_views.py, test_gpu_mser_front.py and test_gpu_parity.py compare the device paths with oracle.detect_msers and
    oracle.detect_describe_views(mser=...); on those images and views the restatement is the reference"""
    need_mser_ref(oracle)
    cases = RC.gpu_suite_cases(oracle)
    assert len(cases) > 100
    total = 0
    for name, img, kw in cases:
        k, tilt, zoom = RC.split_kw(kw)
        ref = oracle.detect_msers_ref(img, tilt=tilt, zoom=zoom, **k)
        _same(oracle.detect_msers(img, tilt=tilt, zoom=zoom, **k), ref, name)
        total += len(ref)
    assert total > 2000


def test_planted_structure_is_there(oracle):
    """what the planted cases claim, read off the reference's own answer"""
    P = RC.planted_groups()
    by = {c[0]: c for g in P.values() for c in g}
    r = _ref(oracle, by["levels/high_levels/p0"])
    assert 2.0 in r["response"][r["sub_type"] == 21]               # the block at 253 on 255: pos 253, margin 2, thresh 254
    r = _ref(oracle, by["area/max_area_99_100_101/p0"])
    assert len(r) == 2 and np.all(r["x"] < 30)                     # 99 and 100 pixels stay, 101 goes
    r = _ref(oracle, by["area/min_size_29_30_31/p0"])
    assert len(r) == 1 and r["x"][0] > 33                          # 31 pixels stay, 29 and 30 go
    assert len(_ref(oracle, by["area/min_size_growing/p0"])) == 3
    r = _ref(oracle, by["promote/striped_130x130/p0"])
    assert len(r) == 1 and r["response"][0] == 188                 # the record starts at level 12 (10000 pixels), not at 20 (12000)
    assert max(len(_ref(oracle, by["levels/rings_0/p%d" % p])) for p in range(3)) >= 3     # one seed, several levels
    plus = _ref(oracle, by["border/edges_corners/p0"])
    plus = plus[plus["sub_type"] == 21]
    assert len(plus) == 8 and plus["x"].min() < 3 and plus["x"].max() > 47 and plus["y"].min() < 3 and plus["y"].max() > 37
    # the tie image: 48 keys of margin 100 and 24 of margin 50 before any cut, and every cut of mode 2 / 3 inside a tie
    tie = RC.tie_image()
    full = oracle.detect_msers_ref(tie, **RC.TIE_BASE, mode=0, min_margin=1.0)
    assert int((full["response"] == 100).sum()) == 48 and int((full["response"] == 50).sum()) == 24
    counts = [len(_ref(oracle, by["ties/blocks72/p%d" % p])) for p in range(len(RC.TIE_PARAMS))]
    n = len(full)
    assert counts[:6] == [17, 60, 40, 100 if n >= 100 else n, int(np.floor(np.float32(0.3) * n)), int(np.floor(np.float32(0.75) * n))]
    assert 0 < counts[0] < 48 and 48 < counts[1] < 72 and 0 < counts[2] < 48 and 0 < counts[4] < 48 and 48 < counts[5] < 72
    assert counts[6] == 48 and counts[7] == 72 and counts[10] == 48 and counts[11] == 72       # a threshold exactly ON the lower tie


def test_trunc_model_is_the_references_conversion(oracle):
    """the reference on f32 pixels == the reference on trunc_u8_model's bytes: (unsigned char)float inside the built reference follows
    the model at every planted value, in the block images and in the blob images of mser_front_cases.trunc_cases()"""
    need_mser_ref(oracle)
    cases = RC.trunc_block_cases() + [("front/" + n, img, MC.MSER_LOOSE) for n, img in MC.trunc_cases().items()]
    assert len(cases) >= 104
    seen = 0
    for name, img, kw in cases:
        u8 = MC.trunc_u8_model(img)
        a = oracle.detect_msers_ref(img, **kw)
        b = oracle.detect_msers_ref(u8.astype(np.float32), **kw)
        _same(a, b, name)
        seen += len(a)
    assert seen > 300


def test_host_pool_views_equal_reference(modsx, oracle):
    """modsx_debug_msers_views_u8 (the engine's MSER step: 2 n (view, polarity) tasks on the host pool) against the reference view by
    view, with per-view tilt and zoom; the pool's threads run the product only, the reference is called here"""
    need_mser_ref(oracle)
    L = modsx.lib()
    picks = ["base_image0/p0", "base_image2/p0", "noise_65x63/p0", "blocked_130x130/p0", "wave_33x200/p0", "nested_200x33/p0",
             "four_levels_17x19/p0", "binary_1x64/p0", "noise_64x1/p0", "noise_2x50/p0", "ties/blocks72/p0", "levels/rings_1/p0",
             "border/edges_corners/p0"]
    by = {c[0]: c for g in GROUPS.values() for c in g}
    imgs = [np.ascontiguousarray(_u8(by[p][1])) for p in picks]
    n = len(imgs)
    tilts = [1.0, 3.0, 1.0, 2.5, 1.0, 1.0, 4.0, 1.0, 1.0, 1.0, 3.0, 1.0, 1.0]
    zooms = [1.0, 1.0, 0.25, 1.0, 0.5, 1.0, 1.0, 1.0, 0.3, 1.0, 1.0, 1.0, 0.4]
    for kw in (dict(min_margin=5.0, min_size=10, max_area=0.2), dict(mode=2, reg_number=60, min_size=5, max_area=0.5)):
        par = modsx.default_mser_params(**kw)
        want = [oracle.detect_msers_ref(g.astype(np.float32), tilt=t, zoom=z, **kw) for g, t, z in zip(imgs, tilts, zooms)]
        assert sum(len(w) for w in want) > 200
        ptrs = (C.c_void_p * n)(*[g.ctypes.data for g in imgs])
        rows = (C.c_int * n)(*[g.shape[0] for g in imgs]); cols = (C.c_int * n)(*[g.shape[1] for g in imgs])
        ct, cz = (C.c_double * n)(*tilts), (C.c_double * n)(*zooms)
        for rep in range(3):
            counts = (C.c_int * n)()
            out = C.c_void_p()
            tot = L.modsx_debug_msers_views_u8(ptrs, rows, cols, n, C.byref(par), ct, cz, counts, C.byref(out))
            assert tot == sum(len(w) for w in want)
            arr = np.frombuffer((C.c_char * (max(tot, 1) * modsx.KEYPOINT.itemsize)).from_address(out.value), dtype=modsx.KEYPOINT,
                                count=tot).copy()
            L.modsx_free(out)
            at = 0
            for i in range(n):
                assert counts[i] == len(want[i]), (rep, picks[i])
                _same(arr[at:at + counts[i]], want[i], (rep, picks[i]))
                at += counts[i]


def test_binding_refuses_tiny_images(oracle):
    """images under 64 pixels never reach the reference (it faults on tiny images; 64 is a margin over the observed line of 30), nor
    does an image of fewer pixels than min(10000, min_size), where its root label is never upgraded to a region"""
    for shape in ((5, 5), (1, 63), (7, 9)):
        with pytest.raises(ValueError):
            oracle.detect_msers_ref(np.zeros(shape, np.float32))
    assert oracle.REF_MSER_MIN_PIXELS == RC.MIN_PIXELS == 64
    for shape, min_size in (((10, 10), 101), ((84, 1), 85), ((90, 100), 20000)):       # fewer pixels than min(10000, min_size)
        with pytest.raises(ValueError):
            oracle.detect_msers_ref(np.zeros(shape, np.float32), min_size=min_size)
    need_mser_ref(oracle)
    assert len(oracle.detect_msers_ref(np.zeros((8, 8), np.float32))) == 0
    k = oracle.detect_msers_ref(RC.tie_image(), **RC.TIE_BASE)
    assert len(k) and np.all(k["octave_number"] == 0) and np.all(k["pyramid_scale"] == 0)      # the unset fields are zero

