"""GPU: the SURF descriptor, bit for bit (uint32 views; entries that are NaN by position) against tests/surf_model.py -- the
restatement of the reference's functor that tests/test_surf_model_cpu.py ties to the compiled reference -- fed with the case
patches or with the oracle's extract_patch / describe_patch(...)[1] patches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fginn32_cases as FC
import surf_cases as Cs
import surf_model as M
from common import oracle_features
from tests import describe_cases as DC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "patchdesc_batch_child.py")
CHILD_TIMEOUT_S = 120          # import + context creation + two calls; what tests/test_gpu_liop.py allows such a child
SIZES = (1, 2, 3, 63, 64, 65)
CHAIN_MR = 20.5                # scale 2: finite rows on real patches


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not len(got):
        return
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN entries differ in rows", list(np.nonzero((np.isnan(got) != nan).any(1))[0][:10]))
    bad = np.nonzero(((u32(got) != u32(ref)) & ~nan).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, (what, "rows that differ:", list(bad[:10]), len(bad))


def _rows(n):
    """n patches: the case list, repeated from its start when n is longer"""
    idx = np.arange(n) % len(Cs.names())
    return Cs.patches()[idx], idx


def _dev(rows, offset):
    """f32 values in a torch buffer on the device, `offset` bytes into it: (keep-alive, device pointer)"""
    import torch
    rows = np.ascontiguousarray(rows, np.float32)
    buf = torch.zeros(rows.size * 4 + 64, dtype=torch.uint8, device="cuda")
    if rows.size:
        buf[offset:offset + rows.size * 4] = torch.from_numpy(rows.reshape(-1).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _back(buf, offset, shape):
    import torch
    torch.cuda.synchronize()
    n = int(np.prod(shape)) * 4
    return buf[offset:offset + n].cpu().numpy().view(np.float32).reshape(shape).copy()


# ---------------------------------------------------------------------------------------------------------- surf_patches
@pytest.mark.parametrize("mr", Cs.MR_SIZES)
def test_surf_patches_from_the_host(ctx, mr):
    ref = Cs.model(mr)
    for n in SIZES + (len(ref),):
        rows, idx = _rows(n)
        same_bits(ctx.surf_patches(rows, mr_size=mr), ref[idx], "mrSize %g, n = %d" % (mr, n))
    same_bits(ctx.surf_patches(Cs.patches().reshape(-1, 1681), mr_size=mr), ref, "flat rows")
    if mr in Cs.MR_NAN:
        assert np.isnan(ref).all()


@pytest.mark.parametrize("mr", Cs.MR_SIZES)
def test_surf_patches_from_device_rows_offset_by_4_bytes(ctx, mr):
    ref = Cs.model(mr)
    for n in SIZES + (len(ref),):
        rows, idx = _rows(n)
        src, sp = _dev(rows, 4)
        dst, dp = _dev(np.zeros((n, 64), np.float32), 4)
        assert sp % 8 == 4 and dp % 8 == 4
        ctx.surf_patches_device(sp, n, dp, mr_size=mr)
        same_bits(_back(dst, 4, (n, 64)), ref[idx], "mrSize %g, n = %d" % (mr, n))
        guard = dst[4 + n * 256:].cpu().numpy()
        assert not guard.any() and not dst[:4].cpu().numpy().any()            # nothing written outside the n rows


def test_two_mr_sizes_alternate_on_one_context(ctx):
    """the table cache: every mrSize gets its own table back, also after more values than the cache has slots"""
    pats = Cs.patches()
    for mr in (5.1962, 20.5, 5.1962, 20.5, 16.4, 30.0, 100.0, 7.0, 5.1962, 20.5):
        want = Cs.model(mr) if mr in Cs.MR_SIZES else M.describe(pats, mr)
        same_bits(ctx.surf_patches(pats, mr_size=mr), want, "mrSize %g" % mr)


# ------------------------------------------------------------------------------------------------- describe_regions_surf
@pytest.fixture(scope="module")
def image(ctx):
    im = ctx.upload(DC.image())
    yield im
    im.free()


@pytest.fixture(scope="module")
def surf_regions():
    """nine regions with small windows, the direct branch among them (the regions tests/test_gpu_liop.py describes)"""
    sizes = tuple(DC.CLASS_SIZE[c] for c in DC.CLASSES) + (0, 19)
    regs = np.concatenate([DC.regions_of(P) if P < 400 else DC.regions_of(P, which=(0,)) for P in sizes])
    regs["id"] = np.arange(len(regs))
    regs = regs[np.nonzero(regs["det_kp"]["s"] <= DC.s_of(77))[0][:9]].copy()
    assert len(regs) == 9
    return regs


@pytest.fixture(scope="module")
def oracle_patches(oracle, surf_regions):
    """{photoNorm: [9][41][41]} of surf_regions on DC.image() at DC.MR_SIZE"""
    raw = np.stack([oracle.extract_patch(DC.image(), surf_regions[i:i + 1], mr_size=DC.MR_SIZE) for i in range(len(surf_regions))])
    return {0: raw, 1: np.stack([oracle.describe_patch(p, photo_norm=1)[1].reshape(41, 41) for p in raw])}


def test_describe_regions_surf(ctx, image, surf_regions, oracle_patches):
    mr = DC.MR_SIZE                 # 1.0: mrSize is used twice, the window and the scale (41: most of the window is outside)
    want = M.describe(oracle_patches[1], mr)
    for n in (0, 1, 2, 3, len(surf_regions)):
        before = ctx.surf_counters()
        got = ctx.describe_regions_surf(image, surf_regions[:n], mr_size=mr)
        d = {k: v - before[k] for k, v in ctx.surf_counters().items()}
        assert got.shape == (n, 64)
        two_step = ctx.surf_patches(ctx.extract_patches(image, surf_regions[:n], mr_size=mr), mr_size=mr)
        same_bits(got, two_step, "n = %d, against surf_patches(extract_patches)" % n)
        same_bits(got, want[:n], "n = %d, against the model on oracle patches" % n)
        assert d == (dict(calls=1, patches=n, sub_batches=1) if n else dict(calls=0, patches=0, sub_batches=0)), d
    dst, dp = _dev(np.zeros((len(surf_regions), 64), np.float32), 4)
    assert ctx.describe_regions_surf(image, surf_regions, mr_size=mr, out_ptr=dp) is None
    same_bits(_back(dst, 4, want.shape), want, "device output")
    dst, dp = _dev(np.zeros((len(surf_regions), 64), np.float32), 4)
    assert ctx.describe_regions_surf_device(image, surf_regions, dp, mr_size=mr) is None
    same_bits(_back(dst, 4, want.shape), want, "describe_regions_surf_device")


def test_describe_regions_surf_on_the_small_pair(ctx, oracle, small_pair):
    """the small pair's regions, with and without photoNorm and fast extraction, at the mrSize of the chain"""
    a, _, _ = small_pair
    _, rr, _ = oracle_features(oracle, a)
    rr = rr[::max(1, len(rr) // 40)][:40]
    im = ctx.upload(a)
    try:
        for pn in (0, 1):
            raw = [oracle.extract_patch(a, rr[i:i + 1], mr_size=CHAIN_MR) for i in range(len(rr))]
            pats = [oracle.describe_patch(p, photo_norm=1)[1].reshape(41, 41) for p in raw] if pn else raw
            got = ctx.describe_regions_surf(im, rr, mr_size=CHAIN_MR, photo_norm=pn)
            same_bits(got, M.describe(pats, CHAIN_MR), "photoNorm = %d, against the model on oracle patches" % pn)
            for fast in (0, 1):
                got = ctx.describe_regions_surf(im, rr, mr_size=CHAIN_MR, photo_norm=pn, fast=fast)
                lib_pats = ctx.extract_patches(im, rr, mr_size=CHAIN_MR, photo_norm=pn, fast=fast)
                same_bits(got, ctx.surf_patches(lib_pats, mr_size=CHAIN_MR), "photoNorm = %d, fast = %d: two steps" % (pn, fast))
                same_bits(got, M.describe(lib_pats, CHAIN_MR), "photoNorm = %d, fast = %d: the model on the library's patches" % (pn, fast))
    finally:
        im.free()


def test_sub_batches_of_four_in_a_child(ctx, modsx, image, surf_regions, oracle_patches, tmp_path):
    assert not os.environ.get("MODSX_SURF_BATCH"), "this module is about the default sub-batch in the parent"
    mr = DC.MR_SIZE
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, image=DC.image(), regs=np.frombuffer(np.ascontiguousarray(surf_regions, modsx.REGION).tobytes(), np.uint8), mr_size=mr)
    p = subprocess.run([sys.executable, CHILD, "surf", inp, outp], env=dict(os.environ, MODSX_SURF_BATCH="4"), timeout=CHILD_TIMEOUT_S,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode(errors="replace")[-1500:]
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("the SURF sub-batch child ended with status %d; nothing more is started on the GPU.  Its stderr ended:\n%s"
                    % (p.returncode, err), returncode=1)
    assert p.returncode == 0, "the SURF sub-batch child failed with status %d:\n%s" % (p.returncode, err)
    z = np.load(outp)
    assert int(z["batch"]) == 4
    same_bits(z["desc"], M.describe(oracle_patches[1], mr), "9 regions in sub-batches of 4")
    same_bits(z["desc"], ctx.describe_regions_surf(image, surf_regions, mr_size=mr), "child against parent")
    ncase = len(Cs.names())
    same_bits(z["cases"], M.describe(Cs.patches(), mr), "the case list in sub-batches of 4")
    cr, cc = (dict(zip(modsx.SURF_COUNTERS, (int(v) for v in z[k]))) for k in ("counters_regions", "counters_cases"))
    assert cr == dict(calls=1, patches=9, sub_batches=3), cr                  # 4 + 4 + 1: two cuts
    assert cc == dict(calls=1, patches=ncase, sub_batches=(ncase + 3) // 4), cc


# ----------------------------------------------------------------------------------------------------------------- chain
def test_chain_on_small_pair(ctx, modsx, oracle, small_pair):
    """detect -> orient -> describe_regions_surf -> match_regions_f32(dim 64) against the oracle chain fed with model descriptors"""
    a, b, _ = small_pair
    par = modsx.default_pair_params(ransac_seed=1)
    sides = []
    for g in (a, b):
        _, rr, _ = oracle_features(oracle, g)
        pats = [oracle.describe_patch(oracle.extract_patch(g, rr[i:i + 1], mr_size=CHAIN_MR), photo_norm=1)[1].reshape(41, 41)
                for i in range(len(rr))]
        im = ctx.upload(g)
        try:
            k = ctx.detect_affine_keypoints(im, modsx.default_hessaff_params())
            ro = ctx.detect_orientation(im, modsx.detect_affine_regions(k))
            regs = modsx.reproject_regions(ro, np.eye(3), g.shape[1], g.shape[0])
            desc = ctx.describe_regions_surf(im, regs, mr_size=CHAIN_MR)
        finally:
            im.free()
        assert len(regs) == len(rr) > 100
        want = M.describe(pats, CHAIN_MR)
        assert desc.shape == (len(rr), 64) and np.isfinite(want).all()
        same_bits(desc, want, "SURF of the detected regions")
        sides.append((regs, desc, rr, want))
    (g1, d1, r1, m1), (g2, d2, r2, m2) = sides
    got = ctx.match_regions_f32(g1, d1, g2, d2, par)
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    tent = oracle.match_fginn(m1, m2, pos2, par.match_ratio, par.contradDist, par.nn)
    pts = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                    r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = oracle.duplicate_filtering(pts, tent["ratio"], par.duplicateDist, True)
    assert len(tent) > 0, "a chain without a tentative compares empty lists"
    assert got["n_regions"] == (len(r1), len(r2)) and got["n_tentatives"] == len(tent)
    FC.same_tents(got["tentatives"], tent[order[keep]])


# --------------------------------------------------------------------------------------------- the neighbours are untouched
def test_other_descriptors_return_the_same_bytes_around_surf_calls(ctx, image, surf_regions):
    mr = DC.MR_SIZE
    before = (ctx.describe_regions(image, surf_regions, mr_size=mr), ctx.describe_regions_liop(image, surf_regions, mr_size=mr),
              ctx.extract_patches(image, surf_regions, mr_size=mr))
    ctx.describe_regions_surf(image, surf_regions, mr_size=mr)
    ctx.surf_patches(Cs.patches(), mr_size=20.5)
    ctx.describe_regions_surf(image, surf_regions, mr_size=mr, photo_norm=0, fast=1)
    after = (ctx.describe_regions(image, surf_regions, mr_size=mr), ctx.describe_regions_liop(image, surf_regions, mr_size=mr),
             ctx.extract_patches(image, surf_regions, mr_size=mr))
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()


# ----------------------------------------------------------------------------------------------- counters and refusals
def test_counters(ctx, modsx):
    before = ctx.surf_counters()
    assert tuple(before) == modsx.SURF_COUNTERS
    ctx.surf_patches(Cs.patches()[:5], mr_size=20.5)
    src, sp = _dev(Cs.patches()[:3], 0)
    dst, dp = _dev(np.zeros((3, 64), np.float32), 0)
    ctx.surf_patches_device(sp, 3, dp, mr_size=20.5)
    d = {k: v - before[k] for k, v in ctx.surf_counters().items()}
    assert d == dict(calls=2, patches=8, sub_batches=2), d


def test_refusals_leave_the_context_usable(ctx, modsx, image, surf_regions):
    L, h = modsx.lib(), ctx._c()
    regs = np.ascontiguousarray(surf_regions, modsx.REGION)
    pats = Cs.patches()
    for ps in (40, 42, 0):
        for call in (lambda: ctx.describe_regions_surf(image, regs, patch_size=ps), lambda: ctx.surf_patches(pats, patch_size=ps)):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+41"):
                call()
    for mr in (0.0, -1.0, float("nan"), float("inf"), 41.0 / 1025.0):
        for call in (lambda: ctx.describe_regions_surf(image, regs, mr_size=mr), lambda: ctx.surf_patches(pats, mr_size=mr)):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+mrSize"):
                call()
    before = ctx.surf_counters()
    buf = np.zeros(9 * 1681, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    img = C.c_void_p(image.h)
    mr = C.c_double(DC.MR_SIZE)
    assert L.modsx_describe_regions_surf(h, img, p(regs), -1, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_describe_regions_surf(h, img, None, 9, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_describe_regions_surf(h, img, p(regs), 9, mr, 41, 0, 1, None) == -1
    assert L.modsx_describe_regions_surf(h, None, p(regs), 9, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_describe_regions_surf_device(h, img, p(regs), 9, mr, 41, 0, 1, None) == -1
    assert L.modsx_surf_patches(h, p(buf), -1, 41, mr, p(buf)) == -1
    assert L.modsx_surf_patches(h, None, 1, 41, mr, p(buf)) == -1
    assert L.modsx_surf_patches(h, p(buf), 1, 41, mr, None) == -1
    assert L.modsx_surf_patches_device(h, None, 1, 41, mr, None) == -1
    src, sp = _dev(pats[:1], 4)
    assert L.modsx_surf_patches_device(h, C.c_void_p(sp + 1), 1, 41, mr, C.c_void_p(sp)) == -1          # not 4-byte aligned
    assert L.modsx_describe_regions_surf_device(h, img, p(regs), 9, mr, 41, 0, 1, C.c_void_p(sp + 2)) == -1
    assert L.modsx_surf_counters(h, None, 3) == -1
    assert ctx.surf_counters() == before                                      # a refusal launches nothing
    # n == 0 succeeds and writes nothing
    assert ctx.surf_patches(np.zeros((0, 41, 41), np.float32)).shape == (0, 64)
    assert ctx.describe_regions_surf(image, regs[:0]).shape == (0, 64)
    assert ctx.surf_counters() == before
    same_bits(ctx.surf_patches(pats, mr_size=20.5), Cs.model(20.5), "after the refusals")
