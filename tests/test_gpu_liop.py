"""GPU: the normalised patches of the description front end and the LIOP descriptor, bit for bit (uint32 views) against
tests/liop_model.py -- the restatement of vl_liopdesc_process that tests/test_liop_model_cpu.py ties to the compiled reference --
and against the oracle's extract_patch / describe_patch(...)[1] for the patches.

fast_extraction: the oracle's extract_patch is the accurate branch only.  For regions of the direct branch the flag changes
nothing, so fast = 1 is compared with the same oracle patch; for larger regions the fast patch is tied to the oracle through
what the oracle computes FROM a patch: oracle.describe_patch(fast patch without photoNorm) must give the descriptor of
oracle.describe_regions(fast = 1) and the photonormalised patch the library returns for photoNorm = 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fginn32_cases as FC
import liop_cases as Cs
import liop_model as M
from common import oracle_features
from tests import describe_cases as DC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "patchdesc_batch_child.py")
CHILD_TIMEOUT_S = 120          # import + context creation + two calls; the floor tests/test_gpu_describe_chunks.py uses for such a child
SIZES = (1, 2, 3, 63, 64, 65)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.nonzero((u32(got) != u32(ref)).reshape(len(got), -1).any(1))[0] if len(got) else []
    assert len(bad) == 0, (what, "rows that differ:", list(bad[:10]), len(bad))


@pytest.fixture(scope="module")
def model():
    return Cs.model()


@pytest.fixture(scope="module")
def ref(model):
    d = np.stack([m["desc"] for m in model])
    d.setflags(write=False)
    return d


def _rows(n):
    """n patches: the case list, repeated from its start when n is longer"""
    idx = np.arange(n) % len(Cs.cases())
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


# ---------------------------------------------------------------------------------------------------------- liop_patches
def test_liop_patches_from_the_host(ctx, ref):
    for n in SIZES + (len(ref),):
        rows, idx = _rows(n)
        same_bits(ctx.liop_patches(rows), ref[idx], "n = %d" % n)
    same_bits(ctx.liop_patches(Cs.patches().reshape(-1, 1681)), ref, "flat rows")


def test_liop_patches_from_device_rows_offset_by_4_bytes(ctx, ref):
    for n in SIZES + (len(ref),):
        rows, idx = _rows(n)
        src, sp = _dev(rows, 4)
        dst, dp = _dev(np.zeros((n, 144), np.float32), 4)
        assert sp % 8 == 4 and dp % 8 == 4
        ctx.liop_patches_device(sp, n, dp)
        same_bits(_back(dst, 4, (n, 144)), ref[idx], "n = %d" % n)
        guard = dst[4 + n * 576:].cpu().numpy()
        assert not guard.any() and not dst[:4].cpu().numpy().any()            # nothing written outside the n rows


def test_debug_liop_paths_permutations_and_counters(ctx, modsx, model, ref):
    before = ctx.liop_counters()
    got = ctx.debug_liop(Cs.patches())
    after = ctx.liop_counters()
    same_bits(got["desc"], ref)
    want_path = np.array([1 if m["straddle"] else 0 for m in model])
    assert np.array_equal(got["path"], want_path)
    ranks = np.minimum(np.arange(M.NPIX) // M.BIN_AREA, M.NBINS - 1)
    for (name, _), m, path, perm in zip(Cs.cases(), model, got["path"], got["perm"]):
        assert sorted(perm.tolist()) == list(range(M.NPIX)), name
        if path:
            assert np.array_equal(perm, m["perm"]), name                      # the reference's quicksort, replayed
        else:
            bins = np.zeros(M.NPIX, np.int64)
            bins[perm] = ranks
            assert np.array_equal(bins, m["bins"]), name                      # any order by key cuts the same bins
    assert 3 * want_path.sum() >= len(model) and 3 * (len(model) - want_path.sum()) >= len(model)
    d = {k: after[k] - before[k] for k in modsx.LIOP_COUNTERS}
    assert d == dict(calls=1, regions=len(model), exact_path=int(want_path.sum()), sub_batches=1), d


# ------------------------------------------------------------------------------------------------------- extract_patches
# one size per path class of the planner, both sides of the direct-branch boundary (P = 0: s = 7, the direct branch; 19: s = 8)
PATCH_SIZES = tuple(DC.CLASS_SIZE[c] for c in DC.CLASSES) + (0, 19)


def _regions_of(P):
    return DC.regions_of(P) if 0 < P < 400 or P == 0 else DC.regions_of(P, which=(0,))    # the large windows: the interior region


@pytest.fixture(scope="module")
def patch_regions():
    regs = np.concatenate([_regions_of(P) for P in PATCH_SIZES])
    regs["id"] = np.arange(len(regs))
    return regs


@pytest.fixture(scope="module")
def oracle_patches(oracle, patch_regions):
    """{photoNorm: [n][41][41]} of patch_regions on DC.image(): extract_patch, then describe_patch(...)[1]"""
    raw = np.stack([oracle.extract_patch(DC.image(), patch_regions[i:i + 1], mr_size=DC.MR_SIZE) for i in range(len(patch_regions))])
    out = {0: raw, 1: np.stack([oracle.describe_patch(p, photo_norm=1)[1].reshape(41, 41) for p in raw])}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def image(ctx):
    im = ctx.upload(DC.image())
    yield im
    im.free()


def test_patch_regions_cover_the_planner(modsx, patch_regions):
    """read from the planner, not restated: every path class and the direct branch occur"""
    seen = set()
    for i in range(len(patch_regions)):
        c = modsx.describe_plan([patch_regions[i:i + 1]], DC.MR_SIZE)["counters"]
        seen.add("direct" if c["direct_jobs"] else DC.class_of({k: c[k] for k in DC.PER_WINDOW}))
    assert seen == set(DC.CLASSES) | {"direct"}, seen
    assert DC.window_of(DC.DIRECT_S) == 0 and DC.window_of(DC.s_of(19)) == 19


@pytest.mark.parametrize("photo_norm", [0, 1])
def test_extract_patches_against_the_oracle(ctx, image, patch_regions, oracle_patches, photo_norm):
    sift_before = ctx.describe_regions(image, patch_regions, mr_size=DC.MR_SIZE)
    got = ctx.extract_patches(image, patch_regions, mr_size=DC.MR_SIZE, photo_norm=photo_norm)
    same_bits(got, oracle_patches[photo_norm], "photoNorm = %d" % photo_norm)
    if photo_norm:
        assert got.min() >= 0.0 and got.max() <= 255.0 and (got == 255.0).any()          # clamped: ties are real
    # into a device buffer 4 bytes off, and one region at a time (the odd tail of two regions per workgroup)
    dst, dp = _dev(np.zeros((len(patch_regions), 1681), np.float32), 4)
    assert ctx.extract_patches(image, patch_regions, mr_size=DC.MR_SIZE, photo_norm=photo_norm, out_ptr=dp) is None
    same_bits(_back(dst, 4, got.shape), got, "device output")
    for n in (1, 2, 3):
        same_bits(ctx.extract_patches(image, patch_regions[:n], mr_size=DC.MR_SIZE, photo_norm=photo_norm), got[:n], "n = %d" % n)
    sift_after = ctx.describe_regions(image, patch_regions, mr_size=DC.MR_SIZE)
    assert sift_before.tobytes() == sift_after.tobytes()


def test_extract_patches_fast(ctx, oracle, image, patch_regions, oracle_patches):
    direct = np.array([DC.window_of(float(s)) == 0 for s in patch_regions["det_kp"]["s"]])
    assert direct.any() and not direct.all()
    fast = {pn: ctx.extract_patches(image, patch_regions, mr_size=DC.MR_SIZE, fast=1, photo_norm=pn) for pn in (0, 1)}
    for pn in (0, 1):
        same_bits(fast[pn][direct], oracle_patches[pn][direct], "direct branch, photoNorm = %d" % pn)
    big = np.nonzero(~direct)[0]
    assert not np.array_equal(fast[0][big], oracle_patches[0][big])                       # the flag does change these
    want = oracle.describe_regions(DC.image(), patch_regions[big], mr_size=DC.MR_SIZE, fast=1)
    for j, i in enumerate(big):
        desc, normed = oracle.describe_patch(fast[0][i], photo_norm=1)
        assert np.array_equal(desc, want[j]), i
        same_bits(normed.reshape(1, 41, 41), fast[1][i:i + 1], "region %d" % i)


def test_extract_patches_flat_region(ctx, oracle):
    """a window whose deviation is below 1e-4 (a flat part of the image; the blur's taps leave it flat to an ulp or two):
    photometricallyNormalize leaves it as it is.  Its LIOP is all ties"""
    img = DC.image().copy()
    img[40:200, 60:260] = np.float32(77.0)
    regs = DC.regions_of(25, which=(0,))
    raw = oracle.extract_patch(img, regs, mr_size=DC.MR_SIZE)
    normed = oracle.describe_patch(raw, photo_norm=1)[1].reshape(41, 41)
    assert np.array_equal(raw, normed) and float(raw.max() - raw.min()) < 1e-4 and abs(float(raw.mean()) - 77.0) < 1e-3
    im = ctx.upload(img)
    try:
        for pn in (0, 1):
            same_bits(ctx.extract_patches(im, regs, mr_size=DC.MR_SIZE, photo_norm=pn), raw[None], "photoNorm = %d" % pn)
        got = ctx.describe_regions_liop(im, regs, mr_size=DC.MR_SIZE)
        same_bits(got, M.describe([raw]), "LIOP of the flat patch")
    finally:
        im.free()


# ------------------------------------------------------------------------------------------------- describe_regions_liop
@pytest.fixture(scope="module")
def liop_regions(patch_regions):
    """nine regions with small windows, the direct branch among them"""
    s = patch_regions["det_kp"]["s"]
    regs = patch_regions[np.nonzero(s <= DC.s_of(77))[0][:9]].copy()
    assert len(regs) == 9
    return regs


@pytest.fixture(scope="module")
def liop_ref(oracle, liop_regions):
    pats = [oracle.describe_patch(oracle.extract_patch(DC.image(), liop_regions[i:i + 1], mr_size=DC.MR_SIZE), photo_norm=1)[1].reshape(41, 41)
            for i in range(len(liop_regions))]
    return np.stack(pats), M.describe(pats)


def test_describe_regions_liop(ctx, modsx, image, liop_regions, liop_ref):
    pats, want = liop_ref
    for n in (0, 1, 2, 3, len(liop_regions)):
        before = ctx.liop_counters()
        got = ctx.describe_regions_liop(image, liop_regions[:n], mr_size=DC.MR_SIZE)
        d = {k: v - before[k] for k, v in ctx.liop_counters().items()}
        assert got.shape == (n, 144)
        two_step = ctx.liop_patches(ctx.extract_patches(image, liop_regions[:n], mr_size=DC.MR_SIZE))
        same_bits(got, two_step, "n = %d, against liop_patches(extract_patches)" % n)
        same_bits(got, want[:n], "n = %d, against the model on oracle patches" % n)
        assert (d["calls"], d["regions"], d["sub_batches"]) == ((1, n, 1) if n else (0, 0, 0)), d
    dst, dp = _dev(np.zeros((len(liop_regions), 144), np.float32), 4)
    assert ctx.describe_regions_liop(image, liop_regions, mr_size=DC.MR_SIZE, out_ptr=dp) is None
    same_bits(_back(dst, 4, want.shape), want, "device output")
    same_bits(ctx.describe_regions_liop(image, liop_regions, mr_size=DC.MR_SIZE, photo_norm=0),
              M.describe(ctx.extract_patches(image, liop_regions, mr_size=DC.MR_SIZE, photo_norm=0)), "photoNorm = 0")


def test_sub_batches_of_four_in_a_child(ctx, modsx, image, liop_regions, liop_ref, ref, tmp_path):
    assert not os.environ.get("MODSX_LIOP_BATCH"), "this module is about the default sub-batch in the parent"
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, image=DC.image(), regs=np.frombuffer(np.ascontiguousarray(liop_regions, modsx.REGION).tobytes(), np.uint8),
             mr_size=DC.MR_SIZE)
    p = subprocess.run([sys.executable, CHILD, "liop", inp, outp], env=dict(os.environ, MODSX_LIOP_BATCH="4"), timeout=CHILD_TIMEOUT_S,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode(errors="replace")[-1500:]
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("the LIOP sub-batch child ended with status %d; nothing more is started on the GPU.  Its stderr ended:\n%s"
                    % (p.returncode, err), returncode=1)
    assert p.returncode == 0, "the LIOP sub-batch child failed with status %d:\n%s" % (p.returncode, err)
    z = np.load(outp)
    assert int(z["batch"]) == 4
    same_bits(z["desc"], liop_ref[1], "9 regions in sub-batches of 4")
    same_bits(z["desc"], ctx.describe_regions_liop(image, liop_regions, mr_size=DC.MR_SIZE), "child against parent")
    same_bits(z["cases"], ref, "the case list in sub-batches of 4")
    cr, cc = (dict(zip(modsx.LIOP_COUNTERS, (int(v) for v in z[k]))) for k in ("counters_regions", "counters_cases"))
    assert (cr["calls"], cr["regions"], cr["sub_batches"]) == (1, 9, 3), cr         # 4 + 4 + 1: two cuts
    assert (cc["calls"], cc["regions"], cc["sub_batches"]) == (1, len(ref), (len(ref) + 3) // 4), cc


# ----------------------------------------------------------------------------------------------------------------- chain
def test_chain_on_small_pair(ctx, modsx, oracle, small_pair):
    """detect -> orient -> describe_regions_liop -> match_regions_f32 against the oracle chain fed with model descriptors"""
    a, b, _ = small_pair
    par = modsx.default_pair_params(ransac_seed=1)
    sides = []
    for g in (a, b):
        _, rr, _ = oracle_features(oracle, g)
        pats = [oracle.describe_patch(oracle.extract_patch(g, rr[i:i + 1]), photo_norm=1)[1].reshape(41, 41) for i in range(len(rr))]
        im = ctx.upload(g)
        try:
            k = ctx.detect_affine_keypoints(im, modsx.default_hessaff_params())
            ro = ctx.detect_orientation(im, modsx.detect_affine_regions(k))
            regs = modsx.reproject_regions(ro, np.eye(3), g.shape[1], g.shape[0])
            desc = ctx.describe_regions_liop(im, regs)
        finally:
            im.free()
        assert len(regs) == len(rr) > 100
        want = M.describe(pats)
        same_bits(desc, want, "LIOP of the detected regions")
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


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(ctx, modsx, image, liop_regions, ref):
    L, h = modsx.lib(), ctx._c()
    regs = np.ascontiguousarray(liop_regions, modsx.REGION)
    pats = Cs.patches()
    for ps in (40, 42, 0):
        for call in (lambda: ctx.extract_patches(image, regs, patch_size=ps), lambda: ctx.describe_regions_liop(image, regs, patch_size=ps),
                     lambda: ctx.liop_patches(pats, patch_size=ps), lambda: ctx.debug_liop(pats, patch_size=ps)):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+41"):
                call()
    before = ctx.liop_counters()
    buf = np.zeros(9 * 1681, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    img = C.c_void_p(image.h)
    mr = C.c_double(DC.MR_SIZE)
    assert L.modsx_extract_patches(h, img, p(regs), -1, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_extract_patches(h, img, None, 9, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_extract_patches(h, img, p(regs), 9, mr, 41, 0, 1, None) == -1
    assert L.modsx_extract_patches(h, None, p(regs), 9, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_extract_patches_device(h, img, p(regs), 9, mr, 41, 0, 1, None) == -1
    assert L.modsx_describe_regions_liop(h, img, p(regs), -1, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_describe_regions_liop(h, img, None, 9, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_describe_regions_liop(h, img, p(regs), 9, mr, 41, 0, 1, None) == -1
    assert L.modsx_describe_regions_liop_device(h, img, p(regs), 9, mr, 41, 0, 1, None) == -1
    assert L.modsx_liop_patches(h, p(buf), -1, 41, p(buf)) == -1
    assert L.modsx_liop_patches(h, None, 1, 41, p(buf)) == -1
    assert L.modsx_liop_patches(h, p(buf), 1, 41, None) == -1
    assert L.modsx_liop_patches_device(h, None, 1, 41, None) == -1
    src, sp = _dev(pats[:1], 4)
    assert L.modsx_liop_patches_device(h, C.c_void_p(sp + 1), 1, 41, C.c_void_p(sp)) == -1          # not 4-byte aligned
    assert L.modsx_debug_liop(h, p(buf), 1, 41, p(buf), None, None) == -1
    assert L.modsx_liop_counters(h, None, 4) == -1
    assert ctx.liop_counters() == before                                      # a refusal launches nothing
    # n == 0 succeeds and writes nothing
    assert ctx.liop_patches(np.zeros((0, 41, 41), np.float32)).shape == (0, 144)
    assert ctx.extract_patches(image, regs[:0]).shape == (0, 41, 41)
    assert ctx.describe_regions_liop(image, regs[:0]).shape == (0, 144)
    assert ctx.debug_liop(np.zeros((0, 41, 41), np.float32))["path"].shape == (0,)
    assert ctx.liop_counters() == before
    same_bits(ctx.liop_patches(pats), ref, "after the refusals")
