"""CPU: the oracle (oracle/liboracle.so, this project's restatement) against the reference's OWN sources, bit for bit.

oracle/_ref/libhessaff_ref.so is the reference's detectors/helpers.cpp, matching/siftdesc.cpp and detectors/affinedetectors/affine.cpp
compiled in place behind oracle/ref_hessaff_shim.cpp (oracle/Makefile); pyoracle's ref_* functions call it.  Every GPU suite of the
HessianAffine + RootSIFT path compares a kernel with the oracle; this module is what stands behind the oracle on those suites' own
inputs: sift_patch_cases' planted patches, baumberg_cases' jobs, affshape_cases' regions, describe_cases' sampling calls, and the
operands of ref_pin_cases.

Comparison rule: f32 as uint32 and f64 as uint64, so that NaN and -0 count.  No tolerance anywhere.
What the reference does not expose is not compared and is said so where it happens: the state of findAffineShape at a
non-converged exit, and operands on which the reference indexes outside its own tables or buffers (the shim refuses those; the
refusal itself is asserted).  Not pinned here at all: the smoothed branch of DescribeRegions (cv::GaussianBlur), the pyramid, the
orientation functor.
"""
import numpy as np
import pytest

import describe_cases as DC
import ref_pin_cases as RC
import sift_patch_cases as SC
from common import need_hessaff_ref
from tests import affshape_cases as AC
from tests import affshape_model as AM
from tests import baumberg_cases as BC

F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- SIFT patches
FAMILIES = tuple(f for g in SC.GROUPS for f in g)


@pytest.mark.parametrize("family", FAMILIES)
def test_sift_patches_oracle_equals_reference(oracle, family):
    """every planted patch of the family under photo_norm 0 and 1: the normalised patch, the raw histogram (f64), SIFT, RootSIFT,
    HalfSIFT and HalfRootSIFT.  HalfRootSIFT through both of the shim's routes (operator() and the public RootSIFTnorm on the shim's
    fold), which must agree: HalfSIFT can only take the second (see the shim's comment)."""
    need_hessaff_ref(oracle)
    idx = [i for i, c in enumerate(SC.planted()) if c["family"] == family]
    assert len(idx) == SC.family_counts()[family] > 0
    seen = dict(normalised=0, left_alone=0, nan_bins=0, clipped=0, zero_length=0)
    for i in idx:
        case = SC.planted()[i]
        p = case["patch"]
        for pn in (0, 1):
            what = (case["name"], pn)
            rpatch, rsum, rvar = oracle.ref_photo_norm(p) if pn else (p, None, None)
            if pn:
                opatch, osum, ovar = oracle.photo_norm(p)
                assert same_bits(rpatch, opatch) and same_bits(rsum, osum) and same_bits(rvar, ovar), what
                changed = not same_bits(rpatch, p)
                assert changed == (not np.float64(rvar) < 0.0001) or not changed, what
                seen["normalised" if changed else "left_alone"] += 1
            raw = None
            for dt in range(4):
                rdesc, rraw = oracle.ref_sift(rpatch, dt)
                odesc, onorm = oracle.describe_patch(p, photo_norm=pn, rootsift=dt)
                assert same_bits(onorm.reshape(41, 41), rpatch), what + (dt, "patch")
                assert same_bits(rdesc, odesc), what + (dt, "descriptor", np.nonzero(bits(rdesc) != bits(odesc))[0][:8])
                assert raw is None or same_bits(raw, rraw)
                raw = rraw
            via_operator, _ = oracle.ref_sift(rpatch, 3, route=0)
            via_fold, _ = oracle.ref_sift(rpatch, 3, route=1)
            assert same_bits(via_operator, via_fold), what + ("the shim's fold is not the reference's",)
            oraw = oracle.sift_histogram(rpatch)
            assert same_bits(raw, oraw), what + ("raw histogram", np.nonzero(bits(raw) != bits(oraw))[0][:8])
            seen["nan_bins"] += bool(np.isnan(raw).any())
            seen["zero_length"] += not raw.any()
            with np.errstate(all="ignore"):
                seen["clipped"] += bool((raw / np.sqrt((raw * raw).sum()) > 0.2).any())
    if family == "photometric":
        assert seen["normalised"] >= 4 and seen["left_alone"] >= 2, seen          # flat and var_below are left alone
    if family == "magnitude":
        assert seen["nan_bins"] >= 1, seen                                          # the overflow case
    if family == "norm":
        assert seen["zero_length"] >= 1 and seen["clipped"] >= 1, seen


def test_sift_refusals(oracle):
    """what the shim refuses: HalfSIFT through operator() (the reference's clip loop overruns its 64-element vector), the full
    types through the fold route, and patches whose differences could index outside ATAN_LUT"""
    need_hessaff_ref(oracle)
    p = SC.by_name("gather/ordinary")["patch"]
    for dt, route in ((2, 0), (0, 1), (1, 1), (4, 0)):
        with pytest.raises(oracle.RefRefused):
            oracle.ref_sift(p, dt, route=route)
    for bad in (np.nan, np.inf, 3e38):
        q = p.copy()
        q[7, 9] = bad
        with pytest.raises(oracle.RefRefused):
            oracle.ref_sift(q, 1)
    assert oracle.ref_sift(p, 2)[0][64:].sum() == 0 and oracle.ref_sift(p, 2)[0][:64].any()


@pytest.mark.parametrize("max_bin", [0.2, float(F(0.2)), 0.05, 1.0])
def test_sift_max_bin_values(oracle, max_bin):
    """maxBinValue as a parameter (0.2 is the drivers' value, 0.2f the struct's default), on the norm family and some random ones"""
    need_hessaff_ref(oracle)
    idx = [i for i, c in enumerate(SC.planted()) if c["family"] == "norm" or c["name"].startswith("random/white")]
    clipped = 0
    for i in idx:
        p = SC.planted()[i]["patch"]
        for dt in range(4):
            rdesc, _ = oracle.ref_sift(p, dt, max_bin=max_bin)
            odesc, _ = oracle.describe_patch(p, photo_norm=0, rootsift=dt, max_bin=max_bin)
            assert same_bits(rdesc, odesc), (SC.planted()[i]["name"], dt, max_bin)
        raw = oracle.ref_sift(p, 0)[1]
        with np.errstate(all="ignore"):
            clipped += bool((raw / np.sqrt((raw * raw).sum()) > max_bin).any())
    assert clipped > 0 or max_bin >= 1.0


# ------------------------------------------------------------------------------------------------- masks, photometric normalisation
def test_masks(oracle):
    need_hessaff_ref(oracle)
    for size in (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 41):
        assert same_bits(oracle.ref_gauss_mask(size), oracle.gauss_mask(size)), size
    for size in (1, 3, 19, 41, 42, 65):
        for sigma in (0.0, size / 3.0, float(F(size / 3.0)), 1.0, 100.0):
            assert same_bits(oracle.ref_circular_gauss_mask(size, size, sigma), oracle.circular_gauss_mask(size, size, sigma)), (size, sigma)
    assert same_bits(oracle.ref_circular_gauss_mask(5, 9, 0.0), oracle.circular_gauss_mask(5, 9, 0.0))
    m = oracle.ref_circular_gauss_mask(41, 41, 0.0)
    assert m[20, 20] == 1.0 and m[0, 0] == 0.0 and m[20, 0] == 0.0 and m[20, 1] > 0       # zero from radius 20 on
    with pytest.raises(oracle.RefRefused):
        oracle.ref_gauss_mask(18)                    # computeGaussMask writes past an even-sized mask


def test_photometric_normalisation_with_other_masks(oracle):
    """photometricallyNormalize under masks other than DescribeRegions' (a full one, a sparse one, an empty one: 0 / 0), on
    sizes other than 41, with sum and var compared as bits"""
    need_hessaff_ref(oracle)
    rs = np.random.RandomState(6401)
    nan_seen = 0
    for rows, cols in ((41, 41), (19, 19), (5, 9), (1, 1)):
        for k in range(6):
            p = (rs.standard_normal((rows, cols)) * (0.01, 1, 40, 300, 1e4, 1e-5)[k] + (0, 100, -50, 1e6, 0, 90)[k]).astype(F)
            for mask in (np.ones((rows, cols), F), (rs.uniform(size=(rows, cols)) < 0.3).astype(F), np.zeros((rows, cols), F),
                         -np.ones((rows, cols), F)):
                r, o = oracle.ref_photo_norm(p, mask), oracle.photo_norm(p, mask)
                assert all(same_bits(a, b) for a, b in zip(r, o)), (rows, cols, k)
                nan_seen += bool(np.isnan(r[1]))
    assert nan_seen > 0                              # the empty mask: sum = 0 / 0


# ------------------------------------------------------------------------------------------------------------------ atan2LUTff
def test_atan2lutff(oracle):
    need_hessaff_ref(oracle)
    yx, tags = RC.atan2_cases()
    need = {"zero_pp", "zero_pn", "zero_np", "zero_nn", "axis", "diagonal", "subnormal", "one_inf"} | set(RC.ATAN2_REFUSED)
    need |= {("cell", i, o, side) for i in range(1, 256) for o in range(8) for side in (0, 1)}
    have = set().union(*tags)
    assert need <= have, sorted(need - have, key=str)[:10]
    values = set()
    for (y, x), t in zip(yx, tags):
        if t & set(RC.ATAN2_REFUSED):
            with pytest.raises(oracle.RefRefused):
                oracle.ref_atan2lutff(y, x)
            continue
        r, o = oracle.ref_atan2lutff(y, x), F(oracle.atan2lut(y, x))
        assert same_bits(r, o), (float(y), float(x), float(r), float(o))
        values.add(int(bits(r).reshape(-1)[0]))
    # the reference alone: both sides of every boundary are different table entries, so the planted operands do land on both
    for i in (1, 32, 83, 100, 128, 255):
        for o, (sx, sy, swap) in enumerate(RC.OCTANTS):
            got = {}
            for (y, x), t in zip(yx, tags):
                for side in (0, 1):
                    if ("cell", i, o, side) in t:
                        got.setdefault(side, set()).add(int(bits(oracle.ref_atan2lutff(y, x)).reshape(-1)[0]))
            assert len(got[0]) == 1 and len(got[1]) == 1 and got[0] != got[1], (i, o, got)
    assert len(values) > 8 * 250


def test_gradients(oracle):
    need_hessaff_ref(oracle)
    for name, img in RC.gradient_images():
        for r, o in zip(oracle.ref_compute_gradient(img), oracle.compute_gradient(img)):
            assert same_bits(r, o), name
        if name != "tiny":
            for r, o in zip(oracle.ref_grad_mag_ori(img), oracle.grad_mag_ori(img)):
                assert same_bits(r, o), name
    ties = dict(RC.gradient_images())["ties"]
    gx, gy = oracle.ref_compute_gradient(ties)
    assert (gx[1:-1, 1:-1] == gy[1:-1, 1:-1]).all()              # |xg| == |yg|: the `x > y` comparisons fall to their else sides
    assert not oracle.ref_grad_mag_ori(dict(RC.gradient_images())["flat"])[1].any()
    with pytest.raises(oracle.RefRefused):
        oracle.ref_compute_gradient(np.zeros((1, 5), F))
    with pytest.raises(oracle.RefRefused):
        oracle.ref_grad_mag_ori(np.full((5, 5), np.nan, F))


# ------------------------------------------------------------------------------------------------ interpolate and its border checks
def test_interpolate(oracle):
    need_hessaff_ref(oracle)
    imgs, calls = RC.interp_images(), RC.interp_calls()
    rows = RC.check_rows(calls)
    touch_int = oracle.ref_interpolate_check_borders(rows)
    assert np.array_equal(touch_int, oracle.ref_interpolate_check_borders(rows, mat=True))       # the two overloads agree
    assert np.array_equal(touch_int, oracle.interpolate_check_borders_wh(rows))
    seen = {}
    for c, touch in zip(calls, touch_int):
        r, rt = oracle.ref_interpolate(imgs[c["img"]], *c["par"], *c["res"])
        o, ot = oracle.interpolate(imgs[c["img"]], *[float(v) for v in c["par"]], *c["res"])
        assert rt == ot and same_bits(r, o), c
        assert not (rt and not touch)                 # the unchecked branch never reports a border
        kind = "inside" if not touch else ("checked, all inside" if not rt else ("wholly outside" if not r.any() else "straddling"))
        seen.setdefault((c["img"], kind), 0)
        seen[(c["img"], kind)] += 1
        seen.setdefault((c["img"], c["centre"], rt), 0)
        seen[(c["img"], c["centre"], rt)] += 1
    for img in range(3):
        kinds = ("inside", "checked, all inside", "straddling", "wholly outside") if img else ("checked, all inside", "straddling", "wholly outside")
        for kind in kinds:                            # a 3 x 3 image has no window the border test lets through
            assert seen.get((img, kind), 0) > 0, (img, kind, seen)
        for centre in ("inside", "edge_left", "edge_right", "edge_top", "edge_bottom"):
            assert seen.get((img, centre, True), 0) > 0 and (seen.get((img, centre, False), 0) > 0 or (img == 0 and centre != "inside")), (img, centre)
        assert seen.get((img, "outside", True), 0) > 0
    for bad in ((np.nan, 1, 1, 0, 0, 1), (1, 1, np.inf, 0, 0, 1)):
        with pytest.raises(oracle.RefRefused):
            oracle.ref_interpolate(imgs[1], *[float(v) for v in bad], 19, 19)
    with pytest.raises(oracle.RefRefused):
        oracle.ref_interpolate(imgs[1], 5.0, 5.0, 1.0, 0.0, 0.0, 1.0, 4, 4)


def test_interpolate_check_borders_alone(oracle):
    """the sizes the callers other than interpolate pass (even, 0, negative) and corners planted on the compared values"""
    need_hessaff_ref(oracle)
    rows = RC.check_only_rows()
    a, b, o = (oracle.ref_interpolate_check_borders(rows), oracle.ref_interpolate_check_borders(rows, mat=True),
               oracle.interpolate_check_borders_wh(rows))
    assert np.array_equal(a, b) and np.array_equal(a, o)
    assert 0.1 < a.mean() < 0.9
    planted = rows[(rows[:, 4] == 1.0) & (rows[:, 5] == 0.0) & (rows[:, 6] == 0.0) & (rows[:, 7] == 1.0)].reshape(-1, 3, 10)
    flips = sum(len(set(oracle.ref_interpolate_check_borders(t).tolist())) == 2 for t in planted)
    assert flips >= len(planted) // 2                # one f32 step across the compared value changes the answer


def test_describe_cases_sampling(oracle):
    """the interpolate() calls DescribeRegions makes for describe_cases' regions: the fast path and the direct branch whole
    (oracle.describe_regions / extract_patch against the reference's interpolate + photometricallyNormalize + SIFTDescriptor on
    ref_pin_cases.sampling_call's parameters), and the first sampling of the smoothed branch for windows up to 135 (the blur behind
    it is OpenCV's and stays unpinned)"""
    need_hessaff_ref(oracle)
    img = DC.image()
    n_fast = n_direct = n_window = 0
    touched = set()
    lists = [DC.regions_of(P) for P in DC.SIZES + (0,)] + [DC.crafted_regions()[::7]]
    for regs in lists:
        for k in range(len(regs)):
            kp = regs["det_kp"][k]
            par = RC.sampling_call(kp, DC.MR_SIZE, fast=True)
            rp, rt = oracle.ref_interpolate(img, *par, 41, 41)
            op, ot = oracle.interpolate(img, *[float(v) for v in par], 41, 41)
            assert rt == ot and same_bits(rp, op)
            want = oracle.ref_describe_patch(rp, 1, 1)[0]
            got = oracle.describe_regions(img, regs[k:k + 1], mr_size=DC.MR_SIZE, fast=1, photo_norm=1, rootsift=1)[0]
            assert same_bits(want, got), ("fast", k, float(kp["s"]))
            n_fast += 1
            touched.add(("fast", rt))
            par = RC.sampling_call(kp, DC.MR_SIZE, fast=False)
            if par is not None:
                rp, rt = oracle.ref_interpolate(img, *par, 41, 41)
                assert same_bits(rp, oracle.extract_patch(img, regs[k], mr_size=DC.MR_SIZE)), ("direct", k)
                want = oracle.ref_describe_patch(rp, 1, 1)[0]
                assert same_bits(want, oracle.describe_regions(img, regs[k:k + 1], mr_size=DC.MR_SIZE)[0]), ("direct", k)
                n_direct += 1
                touched.add(("direct", rt))
            else:
                P = DC.window_of(float(kp["s"]))
                if P <= 135:
                    par = RC.window_call(kp)
                    rw, rt = oracle.ref_interpolate(img, *par, P, P)
                    ow, ot = oracle.interpolate(img, *[float(v) for v in par], P, P)
                    assert rt == ot and same_bits(rw, ow), ("window", P, k)
                    n_window += 1
                    touched.add(("window", rt))
    assert n_fast >= 3 * (len(DC.SIZES) + 1) and n_direct >= 6 and n_window > 150
    assert touched == {(b, t) for b in ("fast", "direct", "window") for t in (False, True)}


# ----------------------------------------------------------------------------------------------------------- the 2x2 / 3x3 helpers
def test_inv_sqrt(oracle):
    need_hessaff_ref(oracle)
    cases = RC.inv_sqrt_cases()
    assert {t for t, _ in cases} >= {"isotropic", "nearly_singular", "singular", "indefinite", "nan", "random", "tiny_b", "equal_diagonal"}
    out = {}
    for tag, abc in cases:
        r, o = oracle.ref_inv_sqrt(*abc), oracle.inv_sqrt(*abc)
        assert same_bits(r, o), (tag, abc, r, o)
        out.setdefault(tag, []).append(r)
    assert all(np.isnan(r[:3]).any() for r in out["nan"]) and all(np.isnan(r[:3]).any() for r in out["indefinite"])
    assert all(np.isfinite(r).all() and r[3] >= r[4] for r in out["random"])
    assert all(abs(r[3] / r[4] - 1) < 1e-6 and r[1] == 0 for r in out["isotropic"])
    assert any(np.isfinite(r).all() and r[3] / r[4] > 1e3 for r in out["nearly_singular"])         # finite, and far from isotropic


def test_get_eigenvalues(oracle):
    need_hessaff_ref(oracle)
    cases = RC.eigen_cases()
    seen = {}
    for tag, m in cases:
        (rok, rl), (ook, ol) = oracle.ref_get_eigenvalues(*m), oracle.get_eigenvalues(*m)
        assert rok == ook and same_bits(rl, ol), (tag, m)
        seen.setdefault(tag, set()).add(rok)
    assert seen["negative_discriminant"] == {False} and seen["isotropic"] == {True}
    assert seen["nearly_zero_discriminant"] == {False, True}        # both sides of delta1 < 0
    assert seen["nan"] == {True}                                    # NaN < 0 is false: the reference goes on with NaN eigenvalues
    assert seen["random"] == {False, True}


def test_solve_linear3x3(oracle):
    need_hessaff_ref(oracle)
    seen = set()
    for tag, A, b in RC.solve3_cases():
        (rA, rb), (oA, ob) = oracle.ref_solve_linear3x3(A, b), oracle.solve_linear3x3(A, b)
        assert same_bits(rA, oA) and same_bits(rb, ob), (tag, A, b)
        seen.add(tag)
        if tag == "random":
            assert np.allclose(A.reshape(3, 3).astype(np.float64) @ rb, b, atol=1e-2 * (1 + np.abs(rb).max()))
        if tag == "singular":
            assert not np.isfinite(rb).all()
        if tag.startswith("pivot_row"):
            assert rA[0] == A[3 * int(tag[-1])]                      # the pivot row went to the top
    assert seen >= {"random", "pivot_row0", "pivot_row1", "pivot_row2", "tie_pivot", "singular", "nearly_singular", "nan", "isotropic"}


def test_rectify(oracle):
    """the three overloads; the oracle's rectify (rectifyTransformation of synth-detection.cpp, the same statements) equals the
    double ones, the float one equals the double one rounded"""
    need_hessaff_ref(oracle)
    seen = {}
    for tag, m in RC.rectify_cases():
        d, dp, o = oracle.ref_rectify(m, "double"), oracle.ref_rectify(m, "pointer"), oracle.rectify(m)
        assert same_bits(d, dp) and same_bits(d, o), (tag, m)
        mf = tuple(float(F(v)) for v in m)
        with np.errstate(all="ignore"):
            assert same_bits(oracle.ref_rectify(mf, "float"), oracle.ref_rectify(mf, "double").astype(F)), (tag, m)
        seen.setdefault(tag, []).append(d)
    assert all(np.isnan(d).any() for d in seen["nan"] + seen["zero"] + seen["zero_first_row"])
    assert all(not np.isfinite(d).all() for d in seen["singular"])
    assert all(np.isfinite(d).all() and d[1] == 0 and abs(d[0] * d[3] - 1) < 1e-9 for d in seen["random"] + seen["rotation"] + seen["reflection"])
    assert all(np.isfinite(d).all() for d in seen["nearly_singular"])


# ------------------------------------------------------------------------------------------------------------------- Baumberg
def _compare_shapes(ref, orc, what):
    """ref: pyoracle.ref_find_affine_shape_batch; orc: the oracle's report.  The flag on every job; u as bits and iters where the
    reference converged.  At a non-converged exit the reference reports nothing (findAffineShape returns false and never calls
    the callback), so the oracle's u / iters / reason there are NOT compared with anything here -- only the flag is."""
    assert np.array_equal(ref["hit"], orc["ok"]), (what, "flag", np.nonzero(ref["hit"] != orc["ok"])[0][:10])
    h = ref["hit"] == 1
    assert same_bits(ref["u"][h], orc["u"][h]), (what, "u", np.nonzero((bits(ref["u"]) != bits(orc["u"])).any(1) & h)[0][:10])
    assert np.array_equal(ref["iters"][h], orc["iters"][h]), (what, "iters")
    assert (orc["reason"][h] == 0).all() and (orc["reason"][~h] != 0).all()
    return h


def test_baumberg_jobs_oracle_equals_reference(oracle):
    need_hessaff_ref(oracle)
    po, xy = RC.baumberg_jobs()
    planes = BC.planes(oracle)
    ref = oracle.ref_find_affine_shape_batch(planes, po, xy, oracle.default_params())
    h = _compare_shapes(ref, BC.oracle_results(oracle, po, xy), "default parameters")
    for p in range(len(planes)):                     # the condition, from the reference alone: a quarter of every plane's jobs
        m = po == p
        assert 4 * int(h[m].sum()) >= int(m.sum()), ("plane %d: the reference converges on %d of %d jobs" % (p, h[m].sum(), m.sum()))
    n0 = len(BC.jobs()[0])
    assert h[:n0].sum() >= 300 and (~h[:n0]).sum() >= 300
    assert set(np.unique(ref["iters"][h]).tolist()) >= set(range(2, 12)) | {0}           # early and late convergence both


@pytest.mark.parametrize("params", [dict(maxIterations=0), dict(maxIterations=1), dict(maxIterations=2), dict(convergenceThreshold=0.01),
                                    dict(convergenceThreshold=0.3), dict(affInitialSigma=0.8), dict(doBaumberg=0)]
                         + [dict(smmWindowSize=W) for W in (3, 5, 7, 9, 11, 13, 15, 17)], ids=str)
def test_baumberg_parameters_oracle_equals_reference(oracle, params):
    """the parameter values tests/test_gpu_baumberg.py and test_gpu_affshape.py sweep, on the first 500 jobs"""
    need_hessaff_ref(oracle)
    po, xy = BC.subset(500)
    par = oracle.default_params(**params)
    ref = oracle.ref_find_affine_shape_batch(BC.planes(oracle), po, xy, par)
    if params.get("doBaumberg", 1) == 0:
        assert ref["hit"].all() and (ref["u"] == np.array([1, 0, 0, 1], F)).all() and (ref["iters"] == 0).all()
        return
    h = _compare_shapes(ref, BC.oracle_results(oracle, po, xy, **params), str(params))
    assert (h.sum() > 0) == (params.get("maxIterations", 16) > 0)


def test_find_affine_shape_refusals(oracle):
    need_hessaff_ref(oracle)
    po, xy = BC.subset(4)
    planes = BC.planes(oracle)
    with pytest.raises(oracle.RefRefused):
        oracle.ref_find_affine_shape_batch(planes, po, xy, oracle.default_params(), method=1)       # AFF_BMBRG_HESSIAN: cv::SVD
    with pytest.raises(oracle.RefRefused):
        oracle.ref_find_affine_shape_batch(planes, po, xy, oracle.default_params(smmWindowSize=18))
    bad = xy.copy()
    bad[1, 0] = np.nan
    with pytest.raises(oracle.RefRefused):
        oracle.ref_find_affine_shape_batch(planes, po, bad, oracle.default_params())


def test_affshape_regions_oracle_equals_reference(oracle):
    need_hessaff_ref(oracle)
    for i, (img, regs) in enumerate(zip(AC.images(oracle), RC.affshape_lists())):
        ref = RC.reference_affshape(oracle, img, regs)
        _, rep = AM.run(oracle, img, regs)
        assert np.array_equal(ref["border"], rep["border"]), i
        run = ~ref["border"]
        h = _compare_shapes({f: ref[f][run] for f in ("hit", "u", "iters")}, {f: rep[f][run] for f in ("ok", "u", "iters", "reason")},
                            "image %d" % i)
        assert 0 < ref["border"].sum() < len(regs)
        assert 4 * int(h.sum()) >= len(regs), ("image %d: the reference converges on %d of %d regions" % (i, h.sum(), len(regs)))


# ------------------------------------------------------------------------------------------------------------ product host code
def test_product_region_export_and_reprojection(modsx, oracle):
    """modsx_detect_affine_regions rectifies with the statements of rectifyAffineTransformationUpIsUp: its a11 .. a22 are the
    reference's, bit for bit.  modsx_reproject_regions / _touch_boundary keep exactly the regions the reference's
    interpolateCheckBorders lets through (identity H: the reprojected keypoint is the detected one; box = (int)(k s) as
    ReprojectRegions forms it, k = 2 * 3 sqrt 3 or the caller's mrSize).  invSqrt has no host-side caller in the product: it runs
    in the Baumberg kernels only, which tests/test_gpu_ref_pin.py compares with the reference's findAffineShape."""
    need_hessaff_ref(oracle)
    rs = np.random.RandomState(6501)
    n = 400
    k = np.zeros(n, modsx.KEYPOINT)
    k["x"], k["y"], k["s"] = rs.uniform(-5, 1030, n), rs.uniform(-5, 775, n), rs.uniform(0.3, 40, n)
    for f in ("a11", "a22"):
        k[f] = rs.uniform(0.3, 2, n) * rs.choice([-1.0, 1.0], n)
    k["a12"], k["a21"] = rs.uniform(-1, 1, n), rs.uniform(-1, 1, n)
    tags = [m for _, m in RC.rectify_cases()][:20]
    for j, m in enumerate(tags):
        k["a11"][j], k["a12"][j], k["a21"][j], k["a22"][j] = m
    with np.errstate(all="ignore"):
        regs = modsx.detect_affine_regions(k)
    want = np.stack([oracle.ref_rectify([k["a11"][j], k["a12"][j], k["a21"][j], k["a22"][j]], "double") for j in range(n)])
    got = np.stack([regs["det_kp"][f] for f in ("a11", "a12", "a21", "a22")], 1)
    assert same_bits(got, want)
    good = regs[np.isfinite(got).all(1)]
    kp = good["det_kp"]
    w, h = 1024, 768
    for box_k, keep in ((2 * 3.0 * np.sqrt(3.0), modsx.reproject_regions(good, np.eye(3), w, h)),
                        (2.0, modsx.reproject_regions_touch_boundary(good, np.eye(3), w, h, 2.0)),
                        (9.0, modsx.reproject_regions_touch_boundary(good, np.eye(3), w, h, 9.0))):
        f = lambda a: a.astype(F).astype(np.float64)          # noqa: E731
        box = np.trunc(box_k * kp["s"])
        t = np.stack([np.full(len(good), w, np.float64), np.full(len(good), h, np.float64), f(kp["x"]), f(kp["y"]), f(kp["a11"]), f(kp["a12"]),
                      f(kp["a21"]), f(kp["a22"]), box, box], 1)
        inside = (kp["x"] < w) & (kp["y"] < h) & (kp["x"] > 0) & (kp["y"] > 0)
        passes = inside & ~oracle.ref_interpolate_check_borders(t)
        assert np.array_equal(keep["id"], good["id"][passes]), box_k
        assert 0 < passes.sum() < len(good)
    # kmath.hpp's check_borders, the border test the kernels evaluate, in its host build
    rows = np.concatenate([RC.check_only_rows(), RC.check_rows(RC.interp_calls())])
    square = rows[rows[:, 8] == rows[:, 9]]
    want = oracle.ref_interpolate_check_borders(square)
    assert np.array_equal(modsx.check_borders(square[:, :9]), want) and len(square) > 1000 and 0.1 < want.mean() < 0.9
