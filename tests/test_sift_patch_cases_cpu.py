"""The claims of tests/sift_patch_cases.py, proven on the CPU against the oracle and tests/dspsift_model.py, and the tie of
tests/sift_gather_model.py (which gather k_describe takes) to both.  tests/test_gpu_sift_patches.py relies on all of it."""
import os
import re

import numpy as np
import pytest

import dspsift_model as D
import orient_model as OM
import sift_gather_model as G
import sift_patch_cases as SC

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope="module")
def cases():
    return SC.planted()


def full_model(case):
    """the cases whose histogram is computed by dspsift_model itself (the rest: ramps the model proves order-free)"""
    return SC.raw_compared(case)


def test_families_and_counts(cases):
    n = SC.family_counts()
    assert n["ramps"] == 8 * 256 - 4 + 4 + 5 + 1 and n["photometric"] == 6 and n["gather"] == 4
    assert n["magnitude"] == len(SC.MAGNITUDE_E) + 2 and n["norm"] == 2 + 2 * 4 * SC.NORM_SEARCH_COUNT
    assert n["random"] == 4 * SC.RANDOM_PER_KIND + 54
    assert sum(1 for c in cases if full_model(c)) < 700              # what is compared with the 16 ms model stays a few hundred
    for im in SC.images():
        assert im["img"].nbytes < 4 << 20 and np.isfinite(im["img"]).all()
    assert [sum(1 for im in SC.images() if im["group"] == "+".join(g)) for g in SC.GROUPS] == list(SC.IMAGES_PER_GROUP)
    assert SC.image_params() == [(k, pn) for k, im in enumerate(SC.images()) for pn in im["options"]["photo_norm"]]
    assert all(SC.planted()[i]["options"] == im["options"] for im in SC.images() for i in im["cases"])


def test_identity_harness(oracle, cases):
    """oracle.describe_regions on the composed images == oracle.describe_patch on every patch; the blank cells are regions of zeros"""
    for im in SC.images():
        for pn in im["options"]["photo_norm"]:
            for rootsift in (0, 1):
                got = oracle.describe_regions(im["img"], SC.regions(oracle.REGION, im["centres"]), SC.MR_SIZE, fast=SC.FAST, photo_norm=pn,
                                              rootsift=rootsift)
                for q, i in enumerate(im["cases"]):
                    assert np.array_equal(got[q], SC.reference(oracle, i, pn)["desc"][rootsift]), (cases[i]["name"], pn, rootsift)
        for side in ("left", "right"):
            x, y = im[side][0]
            assert not im["img"][y - 20:y + 22, x - 20:x + 22].any()
    # the other setting of the harness, s = 2 and mr_size = 10, and a blank cell's descriptor
    im = next(m for m in SC.images() if m["group"] == "gather+magnitude")
    got = oracle.describe_regions(im["img"], SC.regions(oracle.REGION, im["centres"], s=2.0), 10.0, fast=1, photo_norm=0, rootsift=1)
    assert np.array_equal(got, np.stack([SC.reference(oracle, i, 0)["desc"][1] for i in im["cases"]]))
    blank = oracle.describe_regions(im["img"], SC.regions(oracle.REGION, im["left"][:1]), SC.MR_SIZE, fast=1, photo_norm=1, rootsift=1)
    assert not blank.any()


def test_model_equals_oracle(oracle, cases):
    """photometric normalisation, histogram and f64 norms of the models against the oracle, every case under every option"""
    for i, c in enumerate(cases):
        for pn in c["options"]["photo_norm"]:
            r = SC.reference(oracle, i, pn)
            assert same(G.photo_norm(c["patch"]) if pn else c["patch"], r["patch"]), (c["name"], pn)
            d = r["decision"]
            if full_model(c):
                hist = SC.hist_of(oracle, i, pn)
                if not d["inexact"]:
                    assert np.array_equal(d["order_free"], hist), (c["name"], pn)      # order-free: X / S IS the histogram
            else:
                assert not d["inexact"], c["name"]
                hist = d["order_free"]
            for dt in (0, 1):
                assert np.array_equal(D.describe_f64(hist, dt), r["desc"][dt]), (c["name"], pn, dt)
                t = SC.norm_t(hist, dt)
                with np.errstate(all="ignore"):
                    assert np.array_equal(np.clip(np.where(np.isnan(t), 0.0, np.trunc(t)), 0, 255), r["desc"][dt]), (c["name"], pn, dt)


def test_table_coverage(oracle, cases):
    """the ramps hit every entry of k_describe's oTab under the mask: 8 codes x 256 indices and the special entry"""
    hit = set()
    for c in cases:
        if c["family"] != "ramps":
            continue
        st = G.stages(c["patch"])
        e = st["entry"][st["vv"] > 0]
        hit.update(np.unique(e).tolist())
        if "entry" in c["claim"]:
            code, idx = c["claim"]["entry"]
            assert code * 256 + idx in e, c["name"]
        if c["claim"].get("special"):
            assert 2048 in e, c["name"]
    assert hit == set(range(2049))
    # the table itself: the oracle's atan2lut through the reference's expression, entry by entry
    tab = G.o_table()
    for c in (cases[0], cases[777], SC.by_name("sift/ramp/special_x0_ydown")):
        st = G.stages(c["patch"])
        for y, x, o in list(zip(st["yg"].reshape(-1), st["xg"].reshape(-1), st["o"].reshape(-1)))[::97]:
            ori = F(oracle.atan2lut(float(y), float(x)))
            assert o == F((np.float64(8.0) * (np.float64(ori) + D.TWO_PI)) / D.TWO_PI)
    assert tab[2048] == F(8.0)


def test_atan2lut_case_is_one_function_for_both_kernels(cases):
    """kmath.hpp defines atan2lut_case once, k_orientation and k_describe both call it and neither has a copy; orient_model's
    restatement (tied to k_orientation by the orientation tests) gives the entries the ramps claim"""
    src = {f: open(os.path.join(ROOT, "mods_amd", "csrc", f)).read() for f in ("kmath.hpp", "kernels_orient.hip", "kernels_describe.hip")}
    assert len(re.findall(r"\bbool atan2lut_case\(", src["kmath.hpp"])) == 1
    for f in ("kernels_orient.hip", "kernels_describe.hip"):
        assert re.search(r"=\s*atan2lut_case\(yg?, xg?, code, idx\)", src[f]), f
        assert "bool atan2lut_case(" not in src[f] and '#include "kmath.hpp"' in src[f] or '#include "engine.hpp"' in src[f], f
    for c in cases:
        if c["family"] == "ramps" and c["claim"].get("entry") and "rounded" not in c["name"] and "big_bin" not in c["name"]:
            code, idx, special = OM.atan_case(*(G.stages(c["patch"])[k][20, 20] for k in ("yg", "xg")))
            assert (int(code), int(idx)) == tuple(c["claim"]["entry"]) and not special, c["name"]


def test_triggers(oracle, cases):
    """every trigger is reached by the case named for it and by none of the ordinary ones; where the model says ordered, the
    order-free result really differs for at least one case per reachable trigger; a bin of 2^53 is out of reach"""
    differs = {t: 0 for t in G.TRIGGERS}
    xmax = 0
    for i, c in enumerate(cases):
        for pn in c["options"]["photo_norm"]:
            d = SC.reference(oracle, i, pn)["decision"]
            xmax = max(xmax, int(d["X"].max()))
            assert int(d["X"].max()) < G.BIN_BOUND and not d["triggers"]["big_bin"], c["name"]
            claim = c["claim"].get("inexact")
            if claim is not None and pn in claim:
                if claim[pn] is None:
                    assert not d["inexact"], (c["name"], pn, d["triggers"])
                else:
                    assert d["triggers"][claim[pn]], (c["name"], pn, d["triggers"])
            if c["family"] == "random" and "liop_" not in c["name"]:
                assert not d["inexact"], (c["name"], pn)
            if d["inexact"] and full_model(c) and not same(d["order_free"], SC.hist_of(oracle, i, pn)):
                for t in G.TRIGGERS:
                    differs[t] += d["triggers"][t] and sum(d["triggers"].values()) == 1
    assert differs["not_scalable"] >= 1 and differs["small_term"] >= 1 and differs["big_bin"] == 0, differs
    lo, hi = SC.BIG_BIN_REACHED
    assert lo < float(G.decide(SC.by_name("sift/ramp/big_bin_candidate")["patch"])["X"].max()) / 2.0 ** 53 < hi
    assert xmax < 2 ** 53


def test_magnitude_and_reachable_range(cases):
    """E of the magnitude cases; the reachable range of E and of val over every power of two"""
    for c in cases:
        if c["family"] == "magnitude":
            d = G.decide(c["patch"])
            if "E" in c["claim"]:
                assert d["E"] == c["claim"]["E"] and d["scalable"] == (G.E_MIN <= d["E"] <= G.E_MAX), (c["name"], d["E"])
                assert np.isfinite(d["stages"]["g"]).all()
            if c["claim"].get("overflow"):
                g = d["stages"]["g"]
                assert np.isinf(g).any() and np.isnan(d["stages"]["vv"]).any() and d["mxb"] >= 0x7f800000
    assert G.decide(SC.by_name("gather/subnormal_products")["patch"])["stages"]["g"].max() < 2.0 ** -63       # every product xg * xg is subnormal
    base = SC.magnitude_base()
    mask = D.mask()
    r_min = int(np.argmin(np.where(mask[:, 1] > 0, mask[:, 1], 2)))             # the smallest nonzero mask value lies in column 1
    assert mask[r_min, 1] == mask[mask > 0].min()
    seen_E, seen_val = [], []
    for k in range(-160, 130):
        with np.errstate(all="ignore"):
            probes = [(base.astype(np.float64) * 2.0 ** k).astype(F)]
            for m in (1.0, 1.5, 2.0 - 2.0 ** -23):
                # one gradient pixel each: a bump right of the centre (mask 1 at (20, 20), its other neighbours below it) and a
                # frame pixel, which gives pixel (r_min, 1) its gradient and no other pixel under the mask any
                for rr, cc in ((20, 21), (r_min, 0)):
                    b = np.zeros((SC.PS, SC.PS), F)
                    b[rr, cc] = F(m * 2.0 ** k) if k < 128 else F(np.inf)
                    probes.append(b)
        for p in probes:
            if not np.isfinite(p).all():
                continue
            d = G.decide(p)
            if 0 < d["mxb"] < 0x7f800000:
                seen_E.append(d["E"])
                v = d["stages"]["vv"]
                seen_val += [float(v[v > 0].min()), float(v.max())]
                if d["scalable"]:
                    # no positive val scales to zero or to a subnormal, and every term is a normal number or +0
                    with np.errstate(all="ignore"):
                        sc = v[v > 0] * d["S"]
                    assert (sc >= 2.0 ** -126).all() and d["live"] == int((v > 0).sum())
    assert (min(seen_E), max(seen_E)) == SC.E_REACHABLE
    assert SC.VAL_REACHABLE[0] <= min(seen_val) and max(seen_val) < SC.VAL_REACHABLE[1]
    assert G.E_MAX == SC.E_REACHABLE[1] and G.E_MIN > SC.E_REACHABLE[0]
    src = open(os.path.join(ROOT, "mods_amd", "csrc", "kernels_describe.hip")).read()
    assert "E >= %d && E <= %d;" % (G.E_MIN, G.E_MAX) in src                 # the model's bounds are the kernel's


def test_photometric_claims(oracle, cases):
    for i, c in enumerate(cases):
        if c["family"] != "photometric":
            continue
        norm = SC.reference(oracle, i, 1)["patch"]
        assert same(norm, c["patch"]) != c["claim"]["normalised"], c["name"]
        if "clamps" in c["claim"]:
            assert (norm == 0).any() and (norm == 255).any() and ((norm > 0) & (norm < 255)).any()
    lo, hi = SC.by_name("photo/var_below")["patch"], SC.by_name("photo/var_at_or_above")["patch"]
    ne = np.nonzero(lo != hi)
    assert len(ne[0]) == 1 and int(hi[ne].view(np.uint32)[0]) - int(lo[ne].view(np.uint32)[0]) == 1
    assert np.float64(G.photo_stats(lo)[1]) < 0.0001 <= np.float64(G.photo_stats(hi)[1])
    # the large offset: the f32 running sum rounds at almost every add, and another order gives another mean and another patch
    p = SC.by_name("photo/large_offset")["patch"]
    v = p.reshape(-1)[D.mask().reshape(-1) > 0]
    run = np.cumsum(v, dtype=F)
    exact = np.cumsum(v.astype(np.float64))
    assert (run.astype(np.float64) != exact).mean() > 0.9
    assert np.cumsum(v[::-1], dtype=F)[-1] != run[-1]
    blocks = np.cumsum(v[:len(v) & ~3].reshape(-1, 4), 0, dtype=F)[-1]          # four interleaved partial sums, then their sum
    assert len(v) % 4 == 1 and F(np.cumsum(blocks, dtype=F)[-1] + v[-1]) != run[-1]
    assert (SC.by_name("photo/negative")["patch"] < 0).mean() > 0.9


def test_norm_claims(oracle, cases):
    single = SC.by_name("norm/single_pixel")
    d = G.decide(single["patch"])
    h = D.histogram_f64(single["patch"])
    assert d["live"] == 1 and 1 <= (h > 0).sum() <= 8
    v = h / np.sqrt((h * h).sum())
    assert (v > 0.2).any()                                                      # the largest bin clips at max_bin
    zero = SC.by_name("norm/zero_histogram")
    assert not D.histogram_f64(zero["patch"]).any()
    for dt in range(4):
        assert not D.describe_f64(np.zeros(128), dt).any()
        assert np.isnan(SC.norm_t(np.zeros(128), dt)).all()
    sides = {}
    for i, c in enumerate(cases):
        cl = c["claim"].get("rounding")
        if not cl:
            continue
        hist = SC.hist_of(oracle, i, 0)
        t = SC.norm_t(hist, cl["desc_type"])[cl["index"]]
        N = np.float64(cl["N"])
        u = np.spacing(N)
        if cl["side"] == "below":
            assert 0 < N - t <= u, (c["name"], t)
            assert D.describe_f64(hist, cl["desc_type"])[cl["index"]] == N - 1
        else:
            assert 0 <= t - N <= u, (c["name"], t)
            assert D.describe_f64(hist, cl["desc_type"])[cl["index"]] == N
        if cl["desc_type"] < 2:
            assert SC.reference(oracle, i, 0)["desc"][cl["desc_type"]][cl["index"]] == (N - 1 if cl["side"] == "below" else N)
        sides[(cl["desc_type"], cl["side"])] = sides.get((cl["desc_type"], cl["side"]), 0) + 1
    assert sides == {(dt, s): SC.NORM_SEARCH_COUNT for dt in range(4) for s in ("below", "at_or_above")}
    # a pair differs in the last knob alone
    for dt in range(4):
        for k in range(SC.NORM_SEARCH_COUNT):
            a, b = (SC.by_name("norm/round_t%d_%d_%s" % (dt, k, s))["patch"] for s in ("below", "at_or_above"))
            assert [tuple(x) for x in np.argwhere(a != b)] == [SC.ROUND_SITES[1]]


def test_launch_rule():
    """the arrangements of the GPU test pair up as the case module says"""
    im = SC.images()[0]
    n = len(im["centres"])
    assert SC.workgroups(im["centres"]) == [(k, min(k + 1, n - 1)) for k in range(0, n, 2)]
    arr2 = np.stack([im["centres"], im["right"]], 1).reshape(-1, 2)
    arr3 = np.stack([im["left"], im["centres"]], 1).reshape(-1, 2)
    for arr in (arr2, arr3):
        assert SC.workgroups(arr) == [(2 * k, 2 * k + 1) for k in range(n)]
    assert SC.workgroups(im["centres"][:3]) == [(0, 1), (2, 2)]
    assert SC.workgroups(im["centres"][[20, 3, 16]]) == [(1, 2), (0, 0)]         # sorted by band, then x
    assert SC.predicted_ordered(im["centres"][:5], [False, False, True, False, False]) == 1
    assert SC.predicted_ordered(im["centres"][:5], [False, True, True, False, True]) == 3
    img, centres = SC.compose_compact(np.zeros((50, 41, 41), F))
    assert sorted(SC.launch_order(centres).tolist()) == list(range(50)) and img.shape[0] >= centres[:, 1].max() + 22
