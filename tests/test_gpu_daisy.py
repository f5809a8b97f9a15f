"""GPU: the DAISY descriptor, bit for bit (uint32 views) against tests/daisy_model.py -- the restatement of the reference's functor
that tests/test_daisy_model_cpu.py ties to the compiled reference -- fed with the case patches or with the oracle's extract_patch /
describe_patch(...)[1] patches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import daisy_cases as Cs
import daisy_model as M
import fginn32_cases as FC
from common import oracle_features
from tests import describe_cases as DC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "patchdesc_batch_child.py")
CHILD_TIMEOUT_S = 120          # import + context creation + two calls; what tests/test_gpu_surf.py allows such a child
SIZES = (1, 2, 3)              # one workgroup per patch: larger counts repeat the same work
DEFAULT = Cs.PARAMS[0]
INI = Cs.PARAMS[1]
SETS = [(P, nrm) for P in Cs.PARAMS for nrm in Cs.NRMS]
IDS = ["rad%d_radq%d_thq%d_nrm%d" % (P[0], P[1], P[2], nrm) for P, nrm in SETS]
CHAIN_MR = 20.5                # the measurement window of the chain (tests/test_gpu_surf.py)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not len(got):
        return
    assert not np.isnan(ref).any(), what
    bad = np.nonzero((u32(got) != u32(ref)).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, (what, "rows that differ:", list(bad[:10]), len(bad))


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


def kw(P, nrm):
    return dict(rad=P[0], radq=P[1], thq=P[2], histq=P[3], nrm_type=nrm)


# ---------------------------------------------------------------------------------------------------------- daisy_patches
@pytest.mark.parametrize("P,nrm", SETS, ids=IDS)
def test_daisy_patches_from_the_host(ctx, P, nrm):
    ref = Cs.model(P, nrm)
    pats = Cs.patches()
    for n in SIZES + (len(ref),):
        got = ctx.daisy_patches(pats[:n], **kw(P, nrm))
        assert got.shape == (n, M.dim(P[1], P[2]))
        same_bits(got, ref[:n], "%s nrm %d, n = %d" % (P, nrm, n))
    same_bits(ctx.daisy_patches(pats.reshape(-1, 1681), **kw(P, nrm)), ref, "flat rows")


@pytest.mark.parametrize("P,nrm", SETS, ids=IDS)
def test_daisy_patches_from_device_rows_offset_by_4_bytes(ctx, P, nrm):
    ref = Cs.model(P, nrm)
    dim = ref.shape[1]
    for n in SIZES + (len(ref),):
        src, sp = _dev(Cs.patches()[:n], 4)
        dst, dp = _dev(np.zeros((n, dim), np.float32), 4)
        assert sp % 8 == 4 and dp % 8 == 4
        ctx.daisy_patches_device(sp, n, dp, **kw(P, nrm))
        same_bits(_back(dst, 4, (n, dim)), ref[:n], "%s nrm %d, n = %d" % (P, nrm, n))
        guard = dst[4 + n * dim * 4:].cpu().numpy()
        assert not guard.any() and not dst[:4].cpu().numpy().any()            # nothing written outside the n rows


def test_two_triples_alternate_on_one_context(ctx):
    """the table cache: every triple gets its own table back, also after more triples than the cache has slots"""
    pats = Cs.patches()
    extra = ((13, 3, 7, 8), (19, 2, 5, 8))
    for P in (DEFAULT, INI, DEFAULT, INI) + Cs.PARAMS[2:] + extra + (DEFAULT, INI):
        want = Cs.model(P, M.NRM_PARTIAL) if P in Cs.PARAMS else M.describe(pats, *P)
        same_bits(ctx.daisy_patches(pats, **kw(P, M.NRM_PARTIAL)), want, "triple %s" % (P,))


# ------------------------------------------------------------------------------------------------ describe_regions_daisy
@pytest.fixture(scope="module")
def image(ctx):
    im = ctx.upload(DC.image())
    yield im
    im.free()


@pytest.fixture(scope="module")
def daisy_regions():
    """nine regions with small windows, the direct branch among them (the regions tests/test_gpu_surf.py describes)"""
    sizes = tuple(DC.CLASS_SIZE[c] for c in DC.CLASSES) + (0, 19)
    regs = np.concatenate([DC.regions_of(P) if P < 400 else DC.regions_of(P, which=(0,)) for P in sizes])
    regs["id"] = np.arange(len(regs))
    regs = regs[np.nonzero(regs["det_kp"]["s"] <= DC.s_of(77))[0][:9]].copy()
    assert len(regs) == 9
    return regs


@pytest.fixture(scope="module")
def oracle_patches(oracle, daisy_regions):
    """{photoNorm: [9][41][41]} of daisy_regions on DC.image() at DC.MR_SIZE"""
    raw = np.stack([oracle.extract_patch(DC.image(), daisy_regions[i:i + 1], mr_size=DC.MR_SIZE) for i in range(len(daisy_regions))])
    return {0: raw, 1: np.stack([oracle.describe_patch(p, photo_norm=1)[1].reshape(41, 41) for p in raw])}


def test_describe_regions_daisy(ctx, image, daisy_regions, oracle_patches):
    mr = DC.MR_SIZE
    for P, nrm in ((DEFAULT, M.NRM_PARTIAL), (INI, M.NRM_SIFT)):
        want = M.describe(oracle_patches[1], *P, nrm_type=nrm)
        assert np.abs(want).max() > 0
        for n in (0, 1, 2, 3, len(daisy_regions)):
            before = ctx.daisy_counters()
            got = ctx.describe_regions_daisy(image, daisy_regions[:n], mr_size=mr, **kw(P, nrm))
            d = {k: v - before[k] for k, v in ctx.daisy_counters().items()}
            assert got.shape == (n, want.shape[1])
            two_step = ctx.daisy_patches(ctx.extract_patches(image, daisy_regions[:n], mr_size=mr), **kw(P, nrm))
            same_bits(got, two_step, "n = %d, against daisy_patches(extract_patches)" % n)
            same_bits(got, want[:n], "n = %d, against the model on oracle patches" % n)
            assert d == (dict(calls=1, patches=n, sub_batches=1) if n else dict(calls=0, patches=0, sub_batches=0)), d
        dst, dp = _dev(np.zeros(want.shape, np.float32), 4)
        assert ctx.describe_regions_daisy(image, daisy_regions, mr_size=mr, out_ptr=dp, **kw(P, nrm)) is None
        same_bits(_back(dst, 4, want.shape), want, "device output")
        dst, dp = _dev(np.zeros(want.shape, np.float32), 4)
        assert ctx.describe_regions_daisy_device(image, daisy_regions, dp, mr_size=mr, **kw(P, nrm)) is None
        same_bits(_back(dst, 4, want.shape), want, "describe_regions_daisy_device")


def test_describe_regions_daisy_photonorm_and_fast_extraction(ctx, image, daisy_regions, oracle_patches):
    mr = DC.MR_SIZE
    for pn in (0, 1):
        for n in (0, 1, 2, 3):
            got = ctx.describe_regions_daisy(image, daisy_regions[:n], mr_size=mr, photo_norm=pn)
            same_bits(got, M.describe(oracle_patches[pn][:n]), "photoNorm = %d, n = %d, against the model on oracle patches" % (pn, n))
        for fast in (0, 1):
            got = ctx.describe_regions_daisy(image, daisy_regions, mr_size=mr, photo_norm=pn, fast=fast)
            lib_pats = ctx.extract_patches(image, daisy_regions, mr_size=mr, photo_norm=pn, fast=fast)
            same_bits(got, M.describe(lib_pats), "photoNorm = %d, fast = %d: the model on the library's patches" % (pn, fast))
            if not fast:
                same_bits(got, M.describe(oracle_patches[pn]), "photoNorm = %d: the model on oracle patches" % pn)


def test_sub_batches_of_four_in_a_child(ctx, modsx, image, daisy_regions, oracle_patches, tmp_path):
    assert not os.environ.get("MODSX_DAISY_BATCH"), "this module is about the default sub-batch in the parent"
    mr, P, nrm = DC.MR_SIZE, INI, M.NRM_FULL
    order = np.array([5, 2, 8, 0, 7, 3, 1, 6, 4])          # regions out of order: outIdx is no identity inside a sub-batch
    regs = daisy_regions[order]
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, image=DC.image(), regs=np.frombuffer(np.ascontiguousarray(regs, modsx.REGION).tobytes(), np.uint8), mr_size=mr,
             params=np.array(P), nrm_type=nrm)
    p = subprocess.run([sys.executable, CHILD, "daisy", inp, outp], env=dict(os.environ, MODSX_DAISY_BATCH="4"), timeout=CHILD_TIMEOUT_S,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode(errors="replace")[-1500:]
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("the DAISY sub-batch child ended with status %d; nothing more is started on the GPU.  Its stderr ended:\n%s"
                    % (p.returncode, err), returncode=1)
    assert p.returncode == 0, "the DAISY sub-batch child failed with status %d:\n%s" % (p.returncode, err)
    z = np.load(outp)
    assert int(z["batch"]) == 4
    same_bits(z["desc"], M.describe(oracle_patches[1][order], *P, nrm_type=nrm), "9 regions in sub-batches of 4")
    same_bits(z["desc"], ctx.describe_regions_daisy(image, regs, mr_size=mr, **kw(P, nrm)), "child against parent")
    ncase = len(Cs.names())
    same_bits(z["cases"], Cs.model(P, nrm), "the case list in sub-batches of 4")
    cr, cc = (dict(zip(modsx.DAISY_COUNTERS, (int(v) for v in z[k]))) for k in ("counters_regions", "counters_cases"))
    assert cr == dict(calls=1, patches=9, sub_batches=3), cr                  # 4 + 4 + 1: two cuts
    assert cc == dict(calls=1, patches=ncase, sub_batches=(ncase + 3) // 4), cc


# ----------------------------------------------------------------------------------------------------------------- chain
def test_chain_on_small_pair(ctx, modsx, oracle, small_pair):
    """detect -> orient -> describe_regions_daisy -> match_regions_f32(dim 200) against the oracle chain fed with model descriptors"""
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
            desc = ctx.describe_regions_daisy(im, regs, mr_size=CHAIN_MR)
        finally:
            im.free()
        assert len(regs) == len(rr) > 100
        want = M.describe(pats)
        assert desc.shape == (len(rr), 200) and np.isfinite(want).all()
        same_bits(desc, want, "DAISY of the detected regions")
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
def test_other_descriptors_return_the_same_bytes_around_daisy_calls(ctx, image, daisy_regions):
    mr = DC.MR_SIZE
    calls = (lambda: ctx.describe_regions(image, daisy_regions, mr_size=mr), lambda: ctx.describe_regions_surf(image, daisy_regions, mr_size=mr),
             lambda: ctx.describe_regions_liop(image, daisy_regions, mr_size=mr), lambda: ctx.extract_patches(image, daisy_regions, mr_size=mr))
    before = [f() for f in calls]
    ctx.describe_regions_daisy(image, daisy_regions, mr_size=mr)
    ctx.daisy_patches(Cs.patches(), **kw(INI, M.NRM_SIFT))
    ctx.describe_regions_daisy(image, daisy_regions, mr_size=mr, photo_norm=0, fast=1)
    after = [f() for f in calls]
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()


# ----------------------------------------------------------------------------------------------- counters and refusals
def test_counters(ctx, modsx):
    before = ctx.daisy_counters()
    assert tuple(before) == modsx.DAISY_COUNTERS
    ctx.daisy_patches(Cs.patches()[:5])
    src, sp = _dev(Cs.patches()[:3], 0)
    dst, dp = _dev(np.zeros((3, 200), np.float32), 0)
    ctx.daisy_patches_device(sp, 3, dp)
    d = {k: v - before[k] for k, v in ctx.daisy_counters().items()}
    assert d == dict(calls=2, patches=8, sub_batches=2), d


def test_refusals_leave_the_context_usable(ctx, modsx, image, daisy_regions):
    L, h = modsx.lib(), ctx._c()
    regs = np.ascontiguousarray(daisy_regions, modsx.REGION)
    pats = Cs.patches()
    before = ctx.daisy_counters()
    bad = (dict(patch_size=40), dict(patch_size=42), dict(histq=4), dict(histq=9), dict(thq=0), dict(thq=9), dict(radq=0), dict(radq=4),
           dict(rad=0), dict(rad=21), dict(nrm_type=3), dict(nrm_type=-1))
    for k in bad:
        name = "patchSize" if "patch_size" in k else list(k)[0]
        for call in (lambda: ctx.describe_regions_daisy(image, regs, **k), lambda: ctx.daisy_patches(pats, **k)):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+%s" % name):
                call()
    buf = np.zeros(9 * 1681, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    img = C.c_void_p(image.h)
    mr = C.c_double(DC.MR_SIZE)
    tail = (41, 0, 1, 15, 3, 8, 8, 0)
    assert L.modsx_describe_regions_daisy(h, img, p(regs), -1, mr, *tail, p(buf)) == -1
    assert L.modsx_describe_regions_daisy(h, img, None, 9, mr, *tail, p(buf)) == -1
    assert L.modsx_describe_regions_daisy(h, img, p(regs), 9, mr, *tail, None) == -1
    assert L.modsx_describe_regions_daisy(h, None, p(regs), 9, mr, *tail, p(buf)) == -1
    assert L.modsx_describe_regions_daisy_device(h, img, p(regs), 9, mr, *tail, None) == -1
    ptail = (41, 15, 3, 8, 8, 0)
    assert L.modsx_daisy_patches(h, p(buf), -1, *ptail, p(buf)) == -1
    assert L.modsx_daisy_patches(h, None, 1, *ptail, p(buf)) == -1
    assert L.modsx_daisy_patches(h, p(buf), 1, *ptail, None) == -1
    assert L.modsx_daisy_patches_device(h, None, 1, *ptail, None) == -1
    src, sp = _dev(pats[:1], 4)
    assert L.modsx_daisy_patches_device(h, C.c_void_p(sp + 1), 1, *ptail, C.c_void_p(sp)) == -1          # not 4-byte aligned
    assert L.modsx_describe_regions_daisy_device(h, img, p(regs), 9, mr, *tail, C.c_void_p(sp + 2)) == -1
    assert L.modsx_daisy_counters(h, None, 3) == -1
    assert ctx.daisy_counters() == before                                     # a refusal launches nothing
    # n == 0 succeeds and writes nothing
    assert ctx.daisy_patches(np.zeros((0, 41, 41), np.float32)).shape == (0, 200)
    assert ctx.describe_regions_daisy(image, regs[:0]).shape == (0, 200)
    assert ctx.daisy_counters() == before
    same_bits(ctx.daisy_patches(pats, **kw(INI, M.NRM_SIFT)), Cs.model(INI, M.NRM_SIFT), "after the refusals")
