"""The models and cases of tests/mser_front_cases.py, pinned without a device: the truncation rule to the table measured on the
oracle's compiler and to the oracle itself, the sort model to the host path through the component tree, the grey model to the
oracle, and the case list to the residues it claims."""
import numpy as np
import pytest

import mser_front_cases as MC

LOOSE = dict(min_size=1, min_margin=2.0, max_area=1.0)     # the loose parameter set of tests/test_mser_cpu.py


def _same_keys(got, ref):
    assert len(got) == len(ref)
    for f in ref.dtype.names:
        assert np.array_equal(got[f], ref[f]), f


def test_truncation_table():
    """(unsigned char)float on x86, measured with the oracle's compiler (not taken from the kernel)"""
    table = [(-1, 255), (-255, 1), (-256, 0), (-300, 212), (256, 0), (300, 44), (511.9, 255), (2147483520, 128), (2.0 ** 31, 0),
             (1e30, 0), (np.inf, 0), (-np.inf, 0), (np.nan, 0), (-0.5, 0)]
    v = np.array([a for a, _ in table], np.float32)
    assert np.array_equal(MC.trunc_u8_model(v), np.array([b for _, b in table], np.uint8))
    # the rest of the planted list, by the rule: toward zero, low byte; -2^31 is in range (low byte 0), its f32 predecessor is not
    more = [(-0.0, 0), (-0.99, 0), (-1.5, 255), (255, 255), (255.99, 255), (65536, 0), (-2.0 ** 31, 0), (-2147483904, 0),
            (2.0 ** 32, 0), (-1e30, 0)]
    v = np.array([a for a, _ in more], np.float32)
    assert np.array_equal(MC.trunc_u8_model(v), np.array([b for _, b in more], np.uint8))
    # the two lists together are the planted list, bit for bit
    assert set(np.float32([a for a, _ in table + more]).view(np.uint32).tolist()) == set(MC.TRUNC_VALUES.view(np.uint32).tolist())
    # in the byte's own range the rule is numpy's cast
    w = np.linspace(0, 255.996, 4001).astype(np.float32)
    assert np.array_equal(MC.trunc_u8_model(w), w.astype(np.uint8))


@pytest.mark.parametrize("name", sorted(MC.trunc_cases()))
def test_truncation_rule_is_the_oracles(modsx, oracle, name):
    """the oracle truncates the f32 image itself (oracle_mser.cpp:348); the product's host tree on the model's bytes gives the
    same keys only if the model is the oracle's truncation where it matters -- the planted pixels sit inside and beside regions"""
    img = MC.trunc_cases()[name]
    assert (img.size % 4) == int(name[-1])
    for v in MC.TRUNC_VALUES:      # every value is there, bit for bit (NaN and -0.0 included)
        assert np.count_nonzero(img.view(np.uint32) == v.view(np.uint32)) >= 4
    u8 = MC.trunc_u8_model(img)
    for kw in (dict(), LOOSE):
        ref = oracle.detect_msers(img, **kw)
        assert len(ref) >= 20
        _same_keys(modsx.detect_msers_u8(u8, modsx.default_mser_params(**kw)), ref)
    # and the oracle does tell the byte of a planted pixel: the rule's 0 for the values outside int32 against the saturating 255
    sat = u8.copy()
    sat[np.isposinf(img) | (img >= np.float32(2.0 ** 31))] = 255
    ref, alt = oracle.detect_msers(img, **LOOSE), modsx.detect_msers_u8(sat, modsx.default_mser_params(**LOOSE))
    assert len(alt) != len(ref) or any(not np.array_equal(alt[f], ref[f]) for f in ref.dtype.names)


def test_truncation_strips_cover_body_and_tail():
    strips = MC.trunc_strips()
    bits = set(MC.TRUNC_VALUES.view(np.uint32).tolist())
    assert all(s.shape[0] == 1 and s.dtype == np.float32 for s in strips)
    for L in (1, 2, 3):     # the scalar tail alone: every value at every place of it
        for k in range(L):
            assert set(s.view(np.uint32)[0, k] for s in strips if s.shape[1] == L) == bits
    assert any(s.shape[1] == 24 and set(s.view(np.uint32)[0].tolist()) == bits for s in strips)      # the float4 body alone
    for L in (5, 6, 7):
        assert set(np.concatenate([s.view(np.uint32)[0, :4] for s in strips if s.shape[1] == L]).tolist()) == bits


@pytest.mark.parametrize("name", sorted(MC.sort_cases()))
def test_sort_model_and_host_path(modsx, oracle, name):
    img = MC.sort_cases()[name]
    rows, cols = img.shape
    start, order = MC.bin_sort_model(img)
    assert start.shape == (257,) and start[0] == 0 and start[256] == rows * cols and np.all(np.diff(start) >= 0)
    # a permutation of the view's padded offsets, grey levels ascending, raster order inside a level
    rr, cc = np.mgrid[:rows, :cols]
    assert np.array_equal(np.sort(order), np.sort(((rr + 1) * (cols + 2) + cc + 1).ravel()))
    r, c = order // (cols + 2) - 1, order % (cols + 2) - 1
    g = img[r, c].astype(np.int64)
    assert np.all(np.diff(g) >= 0)
    for l in range(256):
        seg = order[start[l]:start[l + 1]]
        assert np.all(g[start[l]:start[l + 1]] == l) and np.all(np.diff(seg) > 0)
    # the host path (its own sort) through the tree: a result exists for every case and is the oracle's
    ref = oracle.detect_msers(img.astype(np.float32), **LOOSE)
    _same_keys(modsx.detect_msers_u8(img, modsx.default_mser_params(**LOOSE)), ref)


def test_gray_model_is_the_oracles(oracle):
    rs = np.random.RandomState(5)
    for shape in ((2, 2), (5, 7), (37, 53), (120, 160)):
        bgr = rs.randint(0, 256, shape + (3,)).astype(np.uint8)
        assert np.array_equal(MC.gray_model(bgr), oracle.gray_from_bgr(bgr))
    # all (B + G, R) pairs that u8 pixels can make
    s, r = np.meshgrid(np.arange(511), np.arange(256))
    bgr = np.stack([np.minimum(s, 255), s - np.minimum(s, 255), r], -1).astype(np.uint8)
    assert np.array_equal(MC.gray_model(bgr), oracle.gray_from_bgr(bgr))
    assert np.array_equal(MC.gray_model(bgr), MC.gray_model(bgr.astype(np.float32)))


def test_engine_cases_give_regions_in_the_oracle(modsx, oracle):
    """what tests/test_gpu_mser_front.py relies on: every edge-image group gives at least 20 regions in the oracle's view loop (the
    step image gives none on its own: DetectOrientation's border test drops the keys of its corner-anchored staircase regions)"""
    cases = MC.engine_cases()
    n = {}
    for name, case in cases.items():
        vo = oracle.set_vs_pars(case["scales"], case["tilts"], case["phi"], case["sigma"], 1, [])
        assert len(vo) == len(modsx.set_vs_pars(case["scales"], case["tilts"], case["phi"], case["sigma"], 1, []))
        regs, desc = oracle.detect_describe_views(case["image"], vo, ori=(5.1962, 41, 1, 0.8), mser=case["mser"], threads=4)
        assert np.isfinite(desc).all()
        n[name] = (len(vo), len(regs))
    assert n["steps_scales"] == (3, 0) and n["ramp_scales"][0] == 3 and n["ramp_scales"][1] >= 20
    assert n["trunc_identity"][0] == 1 and n["trunc_identity"][1] >= 20
    assert n["blob_61_views"][0] == 61 and n["blob_61_views"][1] >= 20
    assert n["blob_51_views"][0] == 51 and n["blob_51_views"][1] >= 20
    # the planted image holds values at which a saturating conversion differs from the rule, and the keys feel it
    img = cases["trunc_identity"]["image"]
    assert np.isfinite(img).all() and np.count_nonzero(img >= np.float32(2.0 ** 31)) >= 8
    sat = MC.trunc_u8_model(img)
    sat[img >= np.float32(2.0 ** 31)] = 255
    ref = oracle.detect_msers(img, **cases["trunc_identity"]["mser"])
    alt = modsx.detect_msers_u8(sat, modsx.default_mser_params(**cases["trunc_identity"]["mser"]))
    assert len(alt) != len(ref) or any(not np.array_equal(alt[f], ref[f]) for f in ref.dtype.names)


def test_case_list_covers_its_residues():
    shapes = [v.shape for v in MC.sort_cases().values()]
    assert {0, 1, 7} <= {r % MC.MSB_ROWS for r, _ in shapes}
    assert {0, 1, 63} <= {c % MC.WAVE for _, c in shapes}
    for want in ((1, 1), (1, 37), (23, 1), (2, 2), (8, 64), (7, 63), (9, 65), (16, 128), (17, 129), (8, 200)):
        assert want in shapes
    s = MC.sort_cases()
    assert np.all(s["constant77_40x50"] == 77) and s["constant77_40x50"].shape == (40, 50)
    c = s["columns_16x256"]
    assert all(len(set(c[r, c0:c0 + 64].tolist())) == 64 for r in range(16) for c0 in range(0, 256, 64))
    rw = s["rows_24x70"]
    assert np.all(rw == rw[:, :1]) and len(set(rw[:, 0].tolist())) == 24 and rw.shape[0] > 2 * MC.MSB_ROWS
    ch = s["checker_0_255_16x130"]
    assert set(np.unique(ch).tolist()) == {0, 255} and all(np.count_nonzero(ch[r, c0:c0 + 64] == 0) == 32 for r in range(16) for c0 in (0, 64))
    assert len(np.unique(s["three_levels_33x100"])) == 3
    n = s["no_0_no_255_20x90"]
    assert n.min() > 0 and n.max() < 255
    b = MC.batch_cases()
    full = b["maxb_mixed"]
    assert len(full) == MC.MAXB and full[MC.MAXB // 2].shape[0] < MC.MSB_ROWS and full[-1].shape == (1, 1)
    assert len({v.shape for v in full}) > 8
    big, small = b["large_then_small"]
    assert big.size > 100 * small.size
    assert sorted(v.size % 4 for v in MC.trunc_cases().values()) == [0, 1, 2, 3]
