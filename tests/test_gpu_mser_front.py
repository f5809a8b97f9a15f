"""GPU: the MSER front end -- k_trunc_u8, the three-launch counting sort k_mser_hist / _scan / _scatter, the block layout and the one
download of mser_front (engine_views.hip) -- per pixel against the numpy models of tests/mser_front_cases.py, all comparisons
exact.  Context.debug_mser_front runs the function the view loop calls, on views the upload path would refuse (one row, one
column, one pixel).

Each case alone; launch sets of mixed sizes up to MAXB views; a large, a small and the large set again on one context (scratch
and staging are reused with another layout); the truncation at every place of the float4 body and of the scalar tail; the engine
path (detect_describe_views, detector 3) on edge images against the oracle's loop; the device sort against the host's sort
(MODSX_MSER_DEVICE_SORT=0 is read once per process: one child, tests/mser_front_child.py); the 3-channel grey ingest.

Fault latch: a child that ends by a signal, with status 134 / 139, by the time limit, or with a failure whose stderr carries a HIP
error sets _FAULT; every later test of this module then fails at once -- no further process, no further use of the context."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mser_front_cases as MC
from common import same_records
from tests import mser_front_child as CH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "mser_front_child.py")
CHILD_CASES = ("ramp_scales", "blob_61_views")
# import, context creation and three launch sets -- about a second of work; the floor of 120 s that tests/test_gpu_match_shapes.py
# derives for such a child applies
CHILD_TIMEOUT_S = 120
HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "device-side assert",
                   "unspecified launch failure", "queue error")
_FAULT = None


def _latch():
    if _FAULT is not None:
        pytest.fail("the host-sort child %s; nothing more is started on the GPU.  Its stderr ended:\n%s" % _FAULT, pytrace=False)


def _f32(u8):
    return u8.astype(np.float32)


def _check_view(got, u8_want, what):
    """one view's (u8, start, order) against the models"""
    u8, start, order = got
    start_want, order_want = MC.bin_sort_model(u8_want)
    assert u8.shape == u8_want.shape and np.array_equal(u8, u8_want), (what, "u8")
    assert np.array_equal(start, start_want), (what, "start")
    assert np.array_equal(order, order_want), (what, "order")


def _same_views(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for k, f in enumerate(("u8", "start", "order")):
            assert np.array_equal(x[k], y[k]), (what, i, f)


@pytest.fixture(scope="module")
def alone(ctx):
    """every sort case in a launch set of its own, computed once"""
    assert os.environ.get("MODSX_MSER_DEVICE_SORT", "1") != "0", "this module is about the device sort being on in the parent"
    _latch()
    out = {}
    for name, img in MC.sort_cases().items():
        out[name] = ctx.debug_mser_front([_f32(img)])[0]
        for a in out[name]:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", sorted(MC.sort_cases()))
def test_each_case_alone(alone, name):
    _latch()
    _check_view(alone[name], MC.sort_cases()[name], name)


@pytest.mark.parametrize("name", sorted(MC.batch_cases()))
def test_batches(ctx, alone, name):
    _latch()
    views = MC.batch_cases()[name]
    got = ctx.debug_mser_front([_f32(v) for v in views])
    assert len(got) == len(views)
    cases = MC.sort_cases()
    for i, v in enumerate(views):
        _check_view(got[i], v, (name, i))
        src = [k for k, c in cases.items() if c.shape == v.shape and np.array_equal(c, v)]      # the sort case this view is
        assert src, (name, i)
        for k, f in enumerate(("u8", "start", "order")):
            assert np.array_equal(got[i][k], alone[src[0]][k]), (name, i, f, "against the view alone")


def test_more_than_maxb_views_is_refused(ctx, modsx):
    _latch()
    one = np.zeros((2, 3), np.float32)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):      # MODSX_ERR_ARG
        ctx.debug_mser_front([one] * (MC.MAXB + 1))
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.debug_mser_front([])
    assert modsx.MAXB == MC.MAXB
    _check_view(ctx.debug_mser_front([one] * MC.MAXB)[-1], np.zeros((2, 3), np.uint8), "MAXB equal views")


def test_buffer_reuse_on_one_context(modsx):
    """a large set, a small one, the large one again on a fresh context: the second and third calls find misc and hMser allocated and
    filled by the call before, with blockHist and start at other offsets"""
    _latch()
    large = [_f32(v) for v in MC.batch_cases()["maxb_mixed"]]
    small = [_f32(v) for v in MC.batch_cases()["large_then_small"][::-1]] + [_f32(MC.sort_cases()["constant77_40x50"])]
    c = modsx.Context(0)
    try:
        first = c.debug_mser_front(large)
        mid = c.debug_mser_front(small)
        again = c.debug_mser_front(large)
        mid2 = c.debug_mser_front(small)
    finally:
        c.close()
    for i, v in enumerate(large):
        _check_view(first[i], v.astype(np.uint8), ("large", i))
    for i, v in enumerate(small):
        _check_view(mid[i], v.astype(np.uint8), ("small", i))
    _same_views(again, first, "large again")
    _same_views(mid2, mid, "small again")


def test_truncation_of_planted_values(ctx):
    """device bytes = the x86 rule at every value, in the float4 body and at every place of the scalar tail; against the unfixed
    kernel ((uint8_t)v, a saturating v_cvt on gfx950) this fails at 2^31, 2^32, 1e30 and +inf: 255 where the rule says 0"""
    _latch()
    for name, img in MC.trunc_cases().items():
        u8 = ctx.debug_mser_front([img])[0][0]
        want = MC.trunc_u8_model(img)
        bad = np.flatnonzero(u8.ravel() != want.ravel())
        print(name, "mismatches", len(bad), [(float(img.ravel()[i]), int(u8.ravel()[i]), int(want.ravel()[i])) for i in bad[:12]])
        assert len(bad) == 0, name
    strips = MC.trunc_strips()
    for s0 in range(0, len(strips), MC.MAXB):
        part = strips[s0:s0 + MC.MAXB]
        got = ctx.debug_mser_front(part)
        for i, s in enumerate(part):
            want = MC.trunc_u8_model(s)
            assert np.array_equal(got[i][0], want), (s0 + i, s.tolist(), got[i][0].tolist(), want.tolist())
            _check_view(got[i], want, ("strip", s0 + i))


def test_single_view_entry_on_planted_values(ctx, modsx, oracle):
    """modsx_detect_msers (k_trunc_u8, then the host's sort and tree) on the whole planted list against the oracle, which truncates
    on the CPU: the stage that is defined for NaN and infinite pixels"""
    _latch()
    for name, img in MC.trunc_cases().items():
        im = ctx.upload(img)
        try:
            got = ctx.detect_msers(im, modsx.default_mser_params(**MC.MSER_LOOSE))
        finally:
            im.free()
        ref = oracle.detect_msers(img, **MC.MSER_LOOSE)
        assert len(ref) >= 20 and same_records(got, ref.view(modsx.KEYPOINT)), name


@pytest.fixture(scope="module")
def engine(ctx, modsx):
    """run_engine of every engine case in this process (device sort on), computed once"""
    _latch()
    return {name: CH.run_engine(modsx, ctx, case) for name, case in MC.engine_cases().items()}


@pytest.fixture(scope="module")
def engine_ref(oracle):
    out = {}
    for name, case in MC.engine_cases().items():
        vo = oracle.set_vs_pars(case["scales"], case["tilts"], case["phi"], case["sigma"], 1, [])
        regs, desc = oracle.detect_describe_views(case["image"], vo, ori=(5.1962, 41, 1, 0.8), mser=case["mser"], threads=8)
        out[name] = (regs, desc, len(vo))
    return out


# The floor of 20 oracle regions holds per edge-image group.  The step image cannot reach it alone under any parameter set: its
# extremal regions are the staircase triangles anchored in two image corners, the oracle finds 26 / 19 / 7 keys in its three views
# and DetectOrientation's border test drops every one of them (0 regions, measured with the oracle).  It runs with the ramp image as
# one group, as the two are listed, and its three views are compared at the front end in test_step_image_views_at_the_front_end.
ENGINE_GROUPS = (("steps_scales", "ramp_scales"), ("trunc_identity",), ("blob_61_views",), ("blob_51_views",))


@pytest.mark.parametrize("group", ENGINE_GROUPS, ids=["+".join(g) for g in ENGINE_GROUPS])
def test_engine_path_on_edge_images(engine, engine_ref, modsx, group):
    _latch()
    total = 0
    for name in group:
        regs, desc, counts = engine[name]
        r_ref, d_ref, nviews = engine_ref[name]
        print(name, "views", nviews, "oracle regions", len(r_ref), "engine regions", len(regs))
        assert len(counts) == nviews and int(counts.sum()) == len(regs)
        assert len(regs) == len(r_ref) and same_records(regs, r_ref.view(modsx.REGION)), name
        assert np.array_equal(desc, d_ref), name
        total += len(r_ref)
    assert total >= 20
    if group[0].startswith("blob_"):
        assert engine_ref[group[0]][2] > MC.MAXB        # two launch sets
    if group[0] == "blob_61_views":
        assert engine_ref[group[0]][2] == 61


def test_step_image_views_at_the_front_end(ctx, oracle):
    """the three views of the step image (90 x 130, 22 x 31, 11 x 15) as one launch set: bytes, level starts and sorted offsets"""
    _latch()
    case = MC.engine_cases()["steps_scales"]
    vo = oracle.set_vs_pars(case["scales"], case["tilts"], case["phi"], case["sigma"], 1, [])
    views = [oracle.synth_view(case["image"], v)[0] for v in vo]
    assert [v.shape for v in views] == [(90, 130), (22, 31), (11, 15)]
    keys = [len(oracle.detect_msers(v, zoom=z, **case["mser"])) for v, z in zip(views, case["scales"])]
    assert min(keys) >= 5 and sum(keys) >= 20, keys       # the views do carry extremal regions
    got = ctx.debug_mser_front(views)
    for i, v in enumerate(views):
        _check_view(got[i], MC.trunc_u8_model(v), ("steps view", i))


@pytest.fixture(scope="module")
def host_sorted(tmp_path_factory):
    """run_engine of CHILD_CASES in a child with MODSX_MSER_DEVICE_SORT=0"""
    global _FAULT
    _latch()
    outp = os.path.join(str(tmp_path_factory.mktemp("mser_front")), "out.npz")
    env = dict(os.environ, MODSX_MSER_DEVICE_SORT="0")
    try:
        p = subprocess.run([sys.executable, CHILD, outp] + list(CHILD_CASES), env=env, timeout=CHILD_TIMEOUT_S, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
    except subprocess.TimeoutExpired as e:
        _FAULT = ("did not end within %d s" % CHILD_TIMEOUT_S, (e.stderr or b"").decode(errors="replace")[-1500:])
        _latch()
    err = p.stderr.decode(errors="replace")[-1500:]
    whole = p.stderr.decode(errors="replace").lower()
    if p.returncode < 0 or p.returncode in (134, 139) or (p.returncode != 0 and any(m in whole for m in HIP_ERROR_MARKS)):
        _FAULT = ("ended with status %d" % p.returncode, err)
        _latch()
    assert p.returncode == 0, "the host-sort child failed with status %d:\n%s" % (p.returncode, err)
    return dict(np.load(outp))


@pytest.mark.parametrize("name", CHILD_CASES)
def test_device_sort_equals_host_sort(engine, host_sorted, modsx, name):
    _latch()
    regs, desc, counts = engine[name]
    assert len(regs) >= 20
    assert same_records(host_sorted[name + "/regs"].view(modsx.REGION), regs)
    assert host_sorted[name + "/desc"].dtype == desc.dtype and host_sorted[name + "/desc"].tobytes() == desc.tobytes()
    assert np.array_equal(host_sorted[name + "/counts"], counts)


def _bgr_cases():
    rs = np.random.RandomState(9)
    out = []
    for shape in ((2, 2), (5, 7), (37, 53)):
        u8 = rs.randint(0, 256, shape + (3,)).astype(np.uint8)
        f32 = (rs.standard_normal(shape + (3,)) * 300.0).astype(np.float32)      # negative values too
        f32.reshape(-1)[::5] = rs.choice(np.float32([1e30, -1e30, 3e38, -3e38, 65536.5, -0.0, 2.0 ** 31]), f32.reshape(-1)[::5].size)
        out.append((u8, f32))
    return out


def test_grey_ingest(ctx, oracle):
    """upload and modsx_image_update of 3-channel u8 and f32 images (B, G, R) against gray_model; n = rows x cols is no multiple of
    the 256 threads of a workgroup; large f32 values overflow B + G to an infinity in the model and on the device alike"""
    _latch()
    for u8, f32 in _bgr_cases():
        assert (u8.shape[0] * u8.shape[1]) % 256 != 0
        assert np.array_equal(MC.gray_model(u8), oracle.gray_from_bgr(u8))
        want_f32 = MC.gray_model(f32)
        assert not np.isnan(want_f32).any()
        for pix, want in ((u8, MC.gray_model(u8)), (f32, want_f32)):
            im = ctx.upload(pix)
            try:
                assert np.array_equal(im.download(), want), (pix.dtype, pix.shape, "upload")
                # two updates on one handle: other pixels of the other type, then the first ones again
                other = f32 if pix is u8 else u8
                im.update(other)
                assert np.array_equal(im.download(), MC.gray_model(other)), (pix.dtype, pix.shape, "update")
                im.update(pix[::-1].copy())
                assert np.array_equal(im.download(), want[::-1]), (pix.dtype, pix.shape, "second update")
            finally:
                im.free()
