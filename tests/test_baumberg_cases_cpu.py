"""CPU: the Baumberg case list (tests/baumberg_cases.py) is fit for its purpose, and the host pieces around the kernels are right.
tests/test_gpu_baumberg.py compares the three Baumberg kernels with the oracle keypoint by keypoint on these cases; this module
proves, without a device, that the cases reach what such a comparison has to reach.

  - Fitness, from oracle.find_affine_shape_batch under the default parameters: every exit of findAffineShape (converged, NaN,
    negative discriminant, anisotropy, iteration limit) and every class of border contact (interpolate()'s border branch on
    every iteration, on none, on some) occurs often enough, converged keypoints leave at many different loop counters, and every
    shape the oracle reports is finite (a NaN shape would send the reference's no-border branch out of bounds).
  - Schedule: with the oracle's iteration counts, the numpy restatement of the stream kernel's slot schedule shows, at chunk
    lengths 3, 5 and 8, a wavefront for every refill pattern of the two slots.  "Both slots take a keypoint in the same pass"
    is met by the first pass of every wavefront; a chunk of 3 has one keypoint left after that pass and cannot show it again, so
    for the chunks of 5 and 8 the pattern is required in a LATER pass as well.
  - Geometry: mods_amd.baumberg_geometry gives the production chunk rule, the grid is padded to the 8 XCDs, and xcd_chunk is a
    bijection of the grid.
  - Borders: mods_amd.check_borders (kmath.hpp, the extrema of the four corners) equals the oracle's interpolateCheckBorders
    (floor / ceil per corner) on more than 10^5 tuples, among them corners exactly on 0, 1, cols - 3 and rows - 3 and one ulp
    either side of each.
"""
import numpy as np
import pytest

from tests import baumberg_cases as BC


@pytest.fixture(scope="module")
def res(oracle):
    return BC.oracle_results(oracle)


def test_case_list_shape():
    po, xy = BC.jobs()
    assert 1200 <= len(po) <= 1300 and xy.shape == (len(po), 4) and xy.dtype == np.float32
    assert np.isfinite(xy).all() and (xy[:, 3] > 0).all()
    # planes are interleaved: the two keypoints a wavefront starts with (chunk >= 2) read planes of different sizes
    shapes = BC.plane_shapes()
    pairs = [(shapes[po[i]], shapes[po[i + 1]]) for i in range(0, len(po) - 1, 2)]
    assert sum(a != b for a, b in pairs) >= 0.9 * len(pairs)
    assert set(po.tolist()) == set(range(len(shapes)))


def test_every_exit_is_reached(res):
    count = dict(zip(BC.REASONS, np.bincount(res["reason"], minlength=5).tolist()))
    print(count)
    assert count["converged"] >= 100 and count["anisotropy"] >= 100 and count["iteration limit"] >= 50
    assert count["negative discriminant"] >= 10 and count["nan"] >= 20
    assert np.array_equal(res["ok"] == 1, res["reason"] == 0)
    assert (res["iters"][res["reason"] == 4] == 16).all() and (res["iters"][res["reason"] != 4] < 16).all()


def test_every_touch_class_is_reached(res):
    t = np.bincount(res["touch"], minlength=4)
    print(t)
    assert t[0] == 0
    assert t[BC.TOUCH_ALWAYS] >= 50 and t[BC.TOUCH_NEVER] >= 50 and t[BC.TOUCH_MIXED] >= 20


def test_converged_keypoints_leave_at_many_loop_counters(res):
    it = res["iters"][res["reason"] == 0]
    print(sorted(set(it.tolist())))
    assert len(set(it.tolist())) >= 10 and it.max() >= 11


def test_every_oracle_coordinate_is_finite(res):
    assert np.isfinite(res["u"]).all()


def test_flat_plane_leaves_by_nan_at_iteration_0(oracle):
    r = oracle.find_affine_shape_batch(BC.planes(oracle), [BC.FLAT], [[20.0, 20.0, 1.6, 1.0]], oracle.default_params())
    assert (r["reason"][0], r["iters"][0], r["ok"][0], r["touch"][0]) == (1, 0, 0, BC.TOUCH_NEVER)
    assert np.array_equal(r["u"][0], np.array([1, 0, 0, 1], np.float32))


def test_batch_entry_equals_the_single_entry(oracle, res):
    """orc_find_affine_shape (the entry the detector's callback uses) against the batch entry, on every 7th job"""
    po, xy = BC.jobs()
    P = BC.planes(oracle)
    par = oracle.default_params()
    for k in range(0, len(po), 7):
        ok, u = oracle.find_affine_shape(P[po[k]], par, *[float(v) for v in xy[k]])
        assert ok == res["ok"][k]
        if ok:
            assert np.array_equal(u, res["u"][k])
    r0 = oracle.find_affine_shape_batch(P, po[:5], xy[:5], oracle.default_params(maxIterations=0))
    assert (r0["iters"] == 0).all() and (r0["ok"] == 0).all() and (r0["reason"] == 4).all()
    assert np.array_equal(r0["u"], np.tile(np.array([1, 0, 0, 1], np.float32), (5, 1)))


@pytest.mark.parametrize("chunk", [3, 5, 8])
def test_schedule_coverage(res, chunk):
    passes = BC.passes_of(res)
    waves = BC.schedule(passes, chunk)
    assert len(waves) == (len(passes) + chunk - 1) // chunk
    seen, later_both = set(), False
    ran = np.zeros(len(passes), np.int64)
    for w in waves:
        seen |= BC.schedule_patterns(w)
        later_both |= any(p > 0 and filled == (0, 1) for p, (_, filled) in enumerate(w))
        assert w[0][1] == ((0, 1) if w[0][0][1] >= 0 else (0,))        # the first pass fills the slots in order
        for job, _ in w:
            for j in job:
                if j >= 0:
                    ran[j] += 1
    assert np.array_equal(ran, passes)                                  # every keypoint runs its iterations, no more
    missing = [p for p in BC.PATTERNS if p not in seen and p != "refill both slots in the same pass"]
    assert not missing, missing
    if chunk >= 4:
        assert later_both


def test_schedule_model_small_cases():
    # chunk 1: slot 1 never fills
    w = BC.schedule([3, 2], 1)
    assert w == [[((0, -1), (0,)), ((0, -1), ()), ((0, -1), ())], [((1, -1), (0,)), ((1, -1), ())]]
    # one wavefront, chunk 4: slot 1 finishes first and takes keypoints 2 and 3 while slot 0 is live; the chunk ends in slot 1
    w = BC.schedule([3, 1, 1, 2], 4)
    assert w == [[((0, 1), (0, 1)), ((0, 2), (1,)), ((0, 3), (1,)), ((-1, 3), ())]]
    assert BC.schedule_patterns(w[0]) == {"refill slot 1 while slot 0 is live", "chunk ends in slot 1"}
    # the mirror image; both slots end in the same pass
    w = BC.schedule([1, 3, 1, 1], 4)
    assert w == [[((0, 1), (0, 1)), ((2, 1), (0,)), ((3, 1), (0,))]]
    assert BC.schedule_patterns(w[0]) == {"refill slot 0 while slot 1 is live"}
    # both slots free in the same pass, then a lone keypoint in slot 0 for four passes
    w = BC.schedule([2, 2, 1, 1, 4], 5)
    assert w == [[((0, 1), (0, 1)), ((0, 1), ()), ((2, 3), (0, 1)), ((4, -1), (0,)), ((4, -1), ()), ((4, -1), ()), ((4, -1), ())]]
    assert BC.schedule_patterns(w[0]) == {"refill both slots in the same pass", "three passes with one slot idle", "chunk ends in slot 0"}


def test_geometry_production_rule(modsx):
    want = {1: 2, 2: 2, 3: 2, 49151: 2, 49152: 3, 131071: 7, 131072: 8, 1000000: 8}
    for n, chunk in want.items():
        g = modsx.baumberg_geometry(n)
        assert g["kernel"] == 0 and g["chunk"] == chunk, (n, g)
        assert g["nchunks"] == (n + chunk - 1) // chunk
        assert g["grid"] % 8 == 0 and g["nchunks"] <= g["grid"] < g["nchunks"] + 8
    for chunk in (1, 2, 3, 5, 8, 13):
        g = modsx.baumberg_geometry(1295, chunk=chunk)
        assert (g["kernel"], g["chunk"], g["nchunks"]) == (0, chunk, (1295 + chunk - 1) // chunk)
    assert modsx.baumberg_geometry(300, variant=1) == dict(kernel=1, chunk=1, nchunks=300, grid=300)
    assert modsx.baumberg_geometry(300, W=19, variant=2)["kernel"] == 2
    assert modsx.baumberg_geometry(300, W=11)["kernel"] == 2 and modsx.baumberg_geometry(300, W=3, variant=2)["grid"] == 300
    for bad in (dict(W=11, variant=1), dict(W=21), dict(W=12), dict(W=1), dict(variant=3), dict(chunk=-1)):
        with pytest.raises(RuntimeError):
            modsx.baumberg_geometry(300, **bad)


def test_xcd_chunk_is_a_bijection_of_the_grid(modsx):
    for n in (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200, 1295):
        for chunk in (1, 2, 3, 8):
            g = modsx.baumberg_geometry(n, chunk=chunk)
            got = sorted(BC.xcd_chunk(b, g["nchunks"]) for b in range(g["grid"]))
            assert got == list(range(g["grid"])), (n, chunk)


def _corner_values(t):
    """the f32 corner coordinates of interpolateCheckBorders for tuples t [n, 9]: -> (x [n, 4], y [n, 4])"""
    f = np.float32
    hw = np.ceil(t[:, 8].astype(f) / 2.0).astype(f)
    xs = np.stack([-hw, -hw, hw, hw], 1)
    ys = np.stack([-hw, hw, -hw, hw], 1)
    c = [t[:, i].astype(f)[:, None] for i in range(9)]
    x = ((c[2] + xs * c[4]).astype(f) + (ys * c[5]).astype(f)).astype(f)
    y = ((c[3] + xs * c[6]).astype(f) + (ys * c[7]).astype(f)).astype(f)
    return x, y


def _border_tuples():
    rs = np.random.RandomState(515)
    out = []
    # random tuples: planes of every size from 4 x 4, centres from outside to outside, any matrix
    n = 60000
    cols, rows = rs.randint(4, 400, n), rs.randint(4, 400, n)
    Wr = 2 * rs.randint(1, 10, n) + 1
    A = rs.normal(0, 1.5, (n, 4))
    out.append(np.column_stack([cols, rows, rs.uniform(-20, cols + 20), rs.uniform(-20, rows + 20), A, Wr]))
    # corners exactly on 0, 1, cols - 3 (x) / rows - 3 (y) and one ulp either side: dyadic matrices keep the corner arithmetic
    # exact, the centre is set so that the extreme corner of one axis lands on the target, the other axis stays inside
    n = 4000
    landed = {}
    for axis in (0, 1):
        for target in ("0", "1", "hi"):
            cols, rows = rs.randint(120, 300, n), rs.randint(120, 300, n)
            Wc = 2 * rs.randint(1, 10, n) + 1
            A = rs.randint(-16, 17, (n, 4)) / 8.0
            A[rs.rand(n, 4) < 0.05] = -0.0
            hw = np.ceil(Wc / 2.0)
            sx = np.stack([-hw, -hw, hw, hw], 1)
            sy = np.stack([-hw, hw, -hw, hw], 1)
            d = sx * A[:, [0 if axis == 0 else 2]] + sy * A[:, [1 if axis == 0 else 3]]       # corner offsets along the axis
            size = cols if axis == 0 else rows
            tv = {"0": np.zeros(n), "1": np.ones(n), "hi": size - 3.0}[target]
            ofs = tv - (d.max(1) if target == "hi" else d.min(1))
            mid = (rows if axis == 0 else cols) * 0.5
            for shift in (-1, 0, 1):
                o = ofs.astype(np.float32)
                if shift:
                    o = np.nextafter(o, np.float32(shift * 1e9))
                ox, oy = (o, mid) if axis == 0 else (mid, o)
                t = np.column_stack([cols, rows, ox, oy, A, Wc]).astype(np.float32)
                out.append(t)
                x, y = _corner_values(t)
                v = x if axis == 0 else y
                ext = v.max(1) if target == "hi" else v.min(1)
                tf = tv.astype(np.float32)
                landed[(axis, target, shift)] = (int((ext < tf).sum()), int((ext == tf).sum()), int((ext > tf).sum()))
    # negative zero everywhere it can stand
    nz = np.float32(-0.0)
    for Wc in range(3, 21, 2):
        for ofs in (nz, np.float32(0.0), np.float32(1.0)):
            out.append(np.array([[64, 48, ofs, ofs, nz, nz, nz, nz, Wc], [64, 48, ofs, 24, 0.5, nz, nz, 0.5, Wc],
                                 [64, 48, 32, ofs, nz, 0.5, 0.5, nz, Wc]], np.float32))
    return np.concatenate([np.asarray(o, np.float32) for o in out]), landed


def test_check_borders_equals_the_reference(modsx, oracle):
    t, landed = _border_tuples()
    assert len(t) >= 100000 and set(t[:, 8].astype(int).tolist()) == set(range(3, 21, 2))
    # the constructed tuples really put the extreme corner below, on and above every target value
    for (axis, target, shift), (lo, eq, hi) in landed.items():
        if shift == 0:
            assert eq >= 3500, (axis, target, shift, lo, eq, hi)
        elif shift < 0:
            assert lo >= 1000, (axis, target, shift, lo, eq, hi)
        else:
            assert hi >= 1000, (axis, target, shift, lo, eq, hi)
    got = modsx.check_borders(t)
    ref = oracle.interpolate_check_borders(t)
    assert 0.2 * len(t) < ref.sum() < 0.8 * len(t)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (len(bad), t[bad[:5]])
