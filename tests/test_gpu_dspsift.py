"""GPU: the raw SIFT histograms, the f32 SIFT norm and DSP-SIFT, bit for bit (uint32 views) against tests/dspsift_model.py -- the
restatement that tests/test_dspsift_model_cpu.py ties to the compiled reference -- fed with the oracle's patches
(extract_patch, then describe_patch(...)[1] for the photometric normalisation).

fast_extraction: the oracle's extract_patch is the accurate branch only.  For regions of the direct branch whose s * mrSize_k is
an integer at every scale the flag changes neither the window nor imageToPatchScale (tests/test_dspsift_model_cpu.py checks that
for dspsift_cases.fast_regions()), so fast = 1 is compared with the same oracle patches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dspsift_cases as Cs
import dspsift_model as M
import fginn32_cases as FC
from common import oracle_features
from tests import describe_cases as DC
from tests import dspsift_chunk_child as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "dspsift_chunk_child.py")
CHILD_TIMEOUT_S = 120          # import + context creation + one call; the floor tests/test_gpu_describe_chunks.py uses for such a child
SIZES = (1, 2, 3, 63, 64, 65)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.nonzero((u32(got) != u32(ref)).reshape(len(got), -1).any(1))[0] if len(got) else []
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


@pytest.fixture(scope="module")
def image(ctx):
    im = ctx.upload(DC.image())
    yield im
    im.free()


# ------------------------------------------------------------------------------------------------------- sift_norm_rows
@pytest.fixture(scope="module")
def norm_ref():
    """{maxBinValue: the model's rows} of the case list"""
    out = {mb: M.sift_norm_f32(Cs.norm_row_array(), mb) for mb in Cs.MAX_BINS}
    for v in out.values():
        v.setflags(write=False)
    return out


def _rows(n):
    """n rows: the case list, repeated from its start when n is longer"""
    idx = np.arange(n) % len(Cs.norm_rows())
    return Cs.norm_row_array()[idx], idx


def test_sift_norm_rows_from_the_host(ctx, norm_ref):
    full = len(Cs.norm_rows())
    assert full > 65
    for mb in Cs.MAX_BINS:
        for n in SIZES + (full,):
            rows, idx = _rows(n)
            same_bits(ctx.sift_norm_rows(rows, max_bin=mb), norm_ref[mb][idx], "n = %d, maxBinValue %r" % (n, mb))
    # every row on its own: nothing of a row depends on its neighbour in the wavefront
    for i, (name, row) in enumerate(Cs.norm_rows()):
        same_bits(ctx.sift_norm_rows(row[None]), norm_ref[0.2][i:i + 1], name)


def test_sift_norm_rows_on_device_rows_offset_by_4_bytes_and_in_place(ctx, norm_ref):
    ref = norm_ref[0.2]
    for n in SIZES + (len(ref),):
        rows, idx = _rows(n)
        src, sp = _dev(rows, 4)
        dst, dp = _dev(np.full((n, 128), -1.0, np.float32), 4)
        assert sp % 8 == 4 and dp % 8 == 4
        ctx.sift_norm_rows_device(sp, n, dp)
        same_bits(_back(dst, 4, (n, 128)), ref[idx], "n = %d" % n)
        same_bits(_back(src, 4, (n, 128)), rows, "n = %d: the input rows are left alone" % n)
        assert not dst[4 + n * 512:].cpu().numpy().any() and not dst[:4].cpu().numpy().any()      # nothing outside the n rows
        # in place, with a row behind the n that must stay as it is
        both = np.concatenate([rows, np.full((1, 128), 7.0, np.float32)])
        buf, bp = _dev(both, 4)
        ctx.sift_norm_rows_device(bp, n, bp)
        got = _back(buf, 4, (n + 1, 128))
        same_bits(got[:n], ref[idx], "n = %d, in place" % n)
        assert (got[n] == 7.0).all() and not buf[:4].cpu().numpy().any() and not buf[4 + (n + 1) * 512:].cpu().numpy().any()


# -------------------------------------------------------------------------------------------------- describe_regions_raw
@pytest.fixture(scope="module")
def raw_ref():
    """{photoNorm: the model's raw histograms of the oracle's patches of raw_regions()}"""
    regs = Cs.raw_regions()
    out = {}
    for pn in (0, 1):
        out[pn] = np.stack([M.raw(Cs.oracle_patch(DC.image(), regs[i:i + 1], DC.MR_SIZE, pn)) for i in range(len(regs))])
        out[pn].setflags(write=False)
    return out


def test_raw_regions_cover_the_planner(modsx):
    """read from the planner, not restated: every path class and the direct branch occur"""
    regs = Cs.raw_regions()
    seen = set()
    for i in range(len(regs)):
        c = modsx.describe_plan([regs[i:i + 1]], DC.MR_SIZE)["counters"]
        seen.add("direct" if c["direct_jobs"] else DC.class_of({k: c[k] for k in DC.PER_WINDOW}))
    assert seen == set(DC.CLASSES) | {"direct"}, seen
    assert DC.window_of(DC.DIRECT_S) == 0 and DC.window_of(DC.s_of(19)) == 19


@pytest.mark.parametrize("photo_norm", [0, 1])
def test_describe_regions_raw_against_the_model(ctx, image, raw_ref, photo_norm):
    regs = Cs.raw_regions()
    sift_before = [ctx.describe_regions(image, regs, mr_size=DC.MR_SIZE, desc_type=t) for t in (0, 1)]
    got = ctx.describe_regions_raw(image, regs, mr_size=DC.MR_SIZE, photo_norm=photo_norm)
    same_bits(got, raw_ref[photo_norm], "photoNorm = %d" % photo_norm)
    assert (got >= 0).all() and (got > 0).any(1).all()
    if photo_norm:
        same_bits(got, Cs.model_raw()[-len(regs):], "the case list's region patches")
    # into a device buffer 4 bytes off, and one to three regions (the odd tail of two regions per workgroup)
    dst, dp = _dev(np.full((len(regs), 128), -1.0, np.float32), 4)
    assert ctx.describe_regions_raw(image, regs, mr_size=DC.MR_SIZE, photo_norm=photo_norm, out_ptr=dp) is None
    same_bits(_back(dst, 4, got.shape), got, "device output")
    assert not dst[:4].cpu().numpy().any() and not dst[4 + got.size * 4:].cpu().numpy().any()
    for n in (1, 2, 3):
        same_bits(ctx.describe_regions_raw(image, regs[:n], mr_size=DC.MR_SIZE, photo_norm=photo_norm), got[:n], "n = %d" % n)
    sift_after = [ctx.describe_regions(image, regs, mr_size=DC.MR_SIZE, desc_type=t) for t in (0, 1)]
    for a, b in zip(sift_before, sift_after):
        assert a.tobytes() == b.tobytes()
    # the histogram is the one the SIFT classes are normalised from
    if photo_norm:
        for i in (0, 5, len(regs) - 1):
            p = Cs.oracle_patch(DC.image(), regs[i:i + 1], DC.MR_SIZE, 1)
            assert np.array_equal(M.describe_f64(M.histogram_f64(p), 0), sift_before[0][i])


def test_describe_regions_raw_flat_window(ctx, oracle):
    """a window without gradients: photometricallyNormalize leaves it alone (deviation below 1e-4) and the histogram holds what
    the blur's last-ulp ripple leaves"""
    img = DC.image().copy()
    img[40:200, 60:260] = np.float32(77.0)
    regs = DC.regions_of(25, which=(0,))
    im = ctx.upload(img)
    try:
        for pn in (0, 1):
            want = M.raw(Cs.oracle_patch(img, regs, DC.MR_SIZE, pn))
            same_bits(ctx.describe_regions_raw(im, regs, mr_size=DC.MR_SIZE, photo_norm=pn), want[None], "photoNorm = %d" % pn)
        same_bits(ctx.describe_regions_dspsift(im, regs, mr_size=DC.MR_SIZE, num_scales=1, start_coef=1.0, end_coef=1.0),
                  M.sift_norm_f32(M.pool([want, want]))[None], "DSP-SIFT of the flat window")
    finally:
        im.free()


# ---------------------------------------------------------------------------------------------- describe_regions_dspsift
_RAW_CACHE = {}


def _model_raw_at(img_key, img, regs, mr, photo_norm=1):
    """the model's raw histograms of regs at measurement size mr, from oracle patches; cached per (image, region, mr)"""
    out = []
    for i in range(len(regs)):
        key = (img_key, regs[i:i + 1].tobytes(), float(mr), photo_norm)
        if key not in _RAW_CACHE:
            _RAW_CACHE[key] = M.raw(Cs.oracle_patch(img, regs[i:i + 1], mr, photo_norm))
        out.append(_RAW_CACHE[key])
    return np.stack(out) if out else np.zeros((0, 128), np.float32)


def _model_dspsift(img_key, img, regs, mr_size, ns, a, b, max_bin=0.2, photo_norm=1):
    if not len(regs):
        return np.zeros((0, 128), np.float32)
    hists = [_model_raw_at(img_key, img, regs, mr, photo_norm) for mr in M.mr_sizes(mr_size, ns, a, b)]
    return M.sift_norm_f32(M.pool(hists), max_bin)


@pytest.fixture(scope="module")
def dsp_ref():
    """{config: the model's descriptors of dsp_regions()}"""
    out = {cfg: _model_dspsift("dc", DC.image(), Cs.dsp_regions(), DC.MR_SIZE, *cfg) for cfg in Cs.CONFIGS}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("config", Cs.CONFIGS, ids=lambda c: "scales%d" % c[0])
def test_describe_regions_dspsift_against_the_model(ctx, modsx, image, dsp_ref, config):
    ns, a, b = config
    regs = Cs.dsp_regions()
    want = dsp_ref[config]
    kw = dict(mr_size=DC.MR_SIZE, num_scales=ns, start_coef=a, end_coef=b)
    for n in (0, 1, 2, 3, len(regs)):
        c0, d0 = ctx.describe_counters(), ctx.dsp_counters()
        got = ctx.describe_regions_dspsift(image, regs[:n], **kw)
        c = {k: v - c0[k] for k, v in ctx.describe_counters().items()}
        d = {k: v - d0[k] for k, v in ctx.dsp_counters().items()}
        assert got.shape == (n, 128)
        same_bits(got, want[:n], "n = %d" % n)
        assert d == (dict(calls=1, regions=n, scale_passes=ns + 1) if n else dict(calls=0, regions=0, scale_passes=0)), d
        assert (c["calls"], c["chunks"], c["jobs"]) == ((ns + 1, ns + 1, n * (ns + 1)) if n else (0, 0, 0)), c
    # the full list: both branches of the front end and at least two planner classes, as the counters of that call show
    if ns > 1:
        assert 0 < c["direct_jobs"] < c["jobs"], c
        assert c["fused_windows"] > 0 and c["jobs"] - c["direct_jobs"] - c["fused_windows"] > 0, c
    assert set(np.unique(got)) <= set(range(256)) and got.max() > 50
    # the whole is its parts: the raw passes pooled on the host, then the norm entry
    hists = [ctx.describe_regions_raw(image, regs, mr_size=float(mr)) for mr in M.mr_sizes(DC.MR_SIZE, ns, a, b)]
    same_bits(ctx.sift_norm_rows(M.pool(hists)), got, "sift_norm_rows of the pooled describe_regions_raw")
    # the device form, 4 bytes off
    dst, dp = _dev(np.full((len(regs), 128), -1.0, np.float32), 4)
    assert ctx.describe_regions_dspsift(image, regs, out_ptr=dp, **kw) is None
    same_bits(_back(dst, 4, want.shape), want, "device output")
    assert not dst[:4].cpu().numpy().any() and not dst[4 + want.size * 4:].cpu().numpy().any()


def test_describe_regions_dspsift_other_parameters(ctx, image, dsp_ref):
    """photoNorm = 0, SIFTDescriptorParams' own clip (double)0.2f, and fast extraction on direct-branch regions"""
    regs = Cs.dsp_regions()[::3]
    ns, a, b = Cs.CONFIGS[1]
    kw = dict(mr_size=DC.MR_SIZE, num_scales=ns, start_coef=a, end_coef=b)
    same_bits(ctx.describe_regions_dspsift(image, regs, photo_norm=0, **kw),
              _model_dspsift("dc", DC.image(), regs, DC.MR_SIZE, ns, a, b, photo_norm=0), "photoNorm = 0")
    mb = Cs.MAX_BINS[1]
    same_bits(ctx.describe_regions_dspsift(image, regs, max_bin=mb, **kw),
              _model_dspsift("dc", DC.image(), regs, DC.MR_SIZE, ns, a, b, max_bin=mb), "maxBinValue = (double)0.2f")
    fast = Cs.fast_regions()
    ns, a, b = Cs.FAST_CONFIG
    want = _model_dspsift("dc", DC.image(), fast, DC.MR_SIZE, ns, a, b)
    for flag in (0, 1):
        c0 = ctx.describe_counters()
        got = ctx.describe_regions_dspsift(image, fast, mr_size=DC.MR_SIZE, fast=flag, num_scales=ns, start_coef=a, end_coef=b)
        c = {k: v - c0[k] for k, v in ctx.describe_counters().items()}
        same_bits(got, want, "fast_extraction = %d" % flag)
        assert c["direct_jobs"] == c["jobs"] == len(fast) * (ns + 1), c


def test_scale_passes_cut_into_chunks_in_a_child(ctx, modsx, tmp_path):
    assert not os.environ.get("MODSX_ARENA_MB"), "this module is about the default arena in the parent"
    one = CC.run(ctx, modsx)
    ns = Cs.CHUNK_CONFIG[0]
    c = dict(zip(modsx.DESCRIBE_COUNTERS, (int(v) for v in one["describe_counters"])))
    assert (c["calls"], c["chunks"]) == (ns + 1, ns + 1), c                   # the parent: one chunk per scale
    outp = str(tmp_path / "out.npz")
    p = subprocess.run([sys.executable, CHILD, outp], env=dict(os.environ, MODSX_ARENA_MB="16"), timeout=CHILD_TIMEOUT_S,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode(errors="replace")[-1500:]
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("the DSP-SIFT chunk child ended with status %d; nothing more is started on the GPU.  Its stderr ended:\n%s"
                    % (p.returncode, err), returncode=1)
    assert p.returncode == 0, "the DSP-SIFT chunk child failed with status %d:\n%s" % (p.returncode, err)
    z = np.load(outp)
    assert int(z["arena_mb"]) == 16
    cc = dict(zip(modsx.DESCRIBE_COUNTERS, (int(v) for v in z["describe_counters"])))
    # the smallest scale fits one chunk, the largest needs several: the cuts differ from scale to scale
    assert cc["calls"] == ns + 1 and cc["chunks"] >= ns + 1 + 4 and cc["chunks_mid_image"] == cc["chunks"] - cc["calls"], cc
    assert cc["jobs"] == c["jobs"] == len(Cs.chunk_regions()) * (ns + 1)
    assert list(z["dsp_counters"]) == list(one["dsp_counters"]) == [1, len(Cs.chunk_regions()), ns + 1]
    same_bits(z["desc"], one["desc"], "chunked scale passes against the one-chunk run")
    assert len(np.unique(one["desc"], axis=0)) == 3                           # three regions, twenty times each


# ----------------------------------------------------------------------------------------------------------------- chain
def test_chain_on_small_pair(ctx, modsx, oracle, small_pair):
    """detect -> orient -> describe_regions_dspsift -> the int8 matcher and match_regions_f32, against the oracle chain fed with
    the model's descriptors"""
    a, b, _ = small_pair
    par = modsx.default_pair_params(ransac_seed=1)
    ns, c0, c1 = Cs.CONFIGS[1]
    sides = []
    for key, g in (("a", a), ("b", b)):
        _, rr, _ = oracle_features(oracle, g)
        im = ctx.upload(g)
        try:
            k = ctx.detect_affine_keypoints(im, modsx.default_hessaff_params())
            ro = ctx.detect_orientation(im, modsx.detect_affine_regions(k))
            regs = modsx.reproject_regions(ro, np.eye(3), g.shape[1], g.shape[0])
            desc = ctx.describe_regions_dspsift(im, regs, num_scales=ns, start_coef=c0, end_coef=c1)
        finally:
            im.free()
        assert len(regs) == len(rr) > 100
        want = _model_dspsift(key, g, rr, 5.1962, ns, c0, c1)
        same_bits(desc, want, "DSP-SIFT of the detected regions")
        sides.append((regs, desc, rr, want))
    (g1, d1, r1, m1), (g2, d2, r2, m2) = sides
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    tent = oracle.match_fginn(m1, m2, pos2, par.match_ratio, par.contradDist, par.nn)
    assert len(tent) > 0, "a chain without a tentative compares empty lists"
    FC.same_tents(ctx.match_fginn(d1, d2, pos2, par.match_ratio, par.contradDist, par.nn), tent)       # the rows are 0..255: int8
    got = ctx.match_regions_f32(g1, d1, g2, d2, par)
    pts = np.stack([r1["reproj_kp"]["x"][tent["q"]], r1["reproj_kp"]["y"][tent["q"]],
                    r2["reproj_kp"]["x"][tent["t0"]], r2["reproj_kp"]["y"][tent["t0"]]], 1)
    order, keep = oracle.duplicate_filtering(pts, tent["ratio"], par.duplicateDist, True)
    assert got["n_regions"] == (len(r1), len(r2)) and got["n_tentatives"] == len(tent)
    FC.same_tents(got["tentatives"], tent[order[keep]])


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(ctx, modsx, image, dsp_ref):
    L, h = modsx.lib(), ctx._c()
    regs = np.ascontiguousarray(Cs.dsp_regions(), modsx.REGION)
    n = len(regs)
    before = (ctx.dsp_counters(), ctx.describe_counters())
    for ps in (40, 42, 0):
        for call in (lambda: ctx.describe_regions_raw(image, regs, patch_size=ps), lambda: ctx.describe_regions_dspsift(image, regs, patch_size=ps)):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+41"):
                call()
    for ns in (0, -1, 65):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+numScales"):
            ctx.describe_regions_dspsift(image, regs, num_scales=ns)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.describe_regions(image, regs, desc_type=4)                         # DSP-SIFT is no descriptor class
    assert ctx.describe_regions_dspsift(image, regs[:1], mr_size=DC.MR_SIZE, num_scales=64, start_coef=1.0, end_coef=1.0).shape == (1, 128)
    before = (ctx.dsp_counters(), ctx.describe_counters())
    # a measurement size that is not finite and positive, at the first scale, in the middle, at the last
    for kw in (dict(mr_size=0.0), dict(mr_size=-1.0), dict(mr_size=float("nan")), dict(mr_size=float("inf")), dict(start_coef=0.0),
               dict(start_coef=-0.5, end_coef=0.5, num_scales=2), dict(start_coef=1.0, end_coef=0.0), dict(end_coef=float("inf")),
               dict(start_coef=float("nan"))):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+finite and positive"):
            ctx.describe_regions_dspsift(image, regs, **kw)
    for mr in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"\(-1\): .+finite and positive"):
            ctx.describe_regions_raw(image, regs, mr_size=mr)
    # a window describe_batch refuses, reached only at the last scale: refused before any scale has run
    big = np.concatenate([regs[:3], DC.regions_of(DC.REFUSED_P - 2, which=(0,))])
    assert DC.window_of(float(big[3]["det_kp"]["s"])) == DC.REFUSED_P - 2
    s_last = float(big[3]["det_kp"]["s"]) * 1.5
    assert DC.window_of(s_last) >= DC.REFUSED_P
    with pytest.raises(RuntimeError, match=r"\(-1\): .+window too large"):
        ctx.describe_regions_dspsift(image, big, mr_size=DC.MR_SIZE, num_scales=3, start_coef=0.5, end_coef=1.5)
    with pytest.raises(RuntimeError, match=r"\(-1\): .+window too large"):
        ctx.describe_regions_raw(image, DC.regions_of(DC.REFUSED_P, which=(0,)), mr_size=DC.MR_SIZE)
    buf = np.zeros(n * 128, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    img, mr, d = C.c_void_p(image.h), C.c_double(DC.MR_SIZE), C.c_double
    dsp = (3, d(0.5), d(1.5), d(0.2))
    assert L.modsx_describe_regions_raw(h, img, p(regs), -1, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_describe_regions_raw(h, img, None, n, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_describe_regions_raw(h, img, p(regs), n, mr, 41, 0, 1, None) == -1
    assert L.modsx_describe_regions_raw(h, None, p(regs), n, mr, 41, 0, 1, p(buf)) == -1
    assert L.modsx_describe_regions_raw_device(h, img, p(regs), n, mr, 41, 0, 1, None) == -1
    assert L.modsx_describe_regions_dspsift(h, img, p(regs), -1, mr, 41, 0, 1, *dsp, p(buf)) == -1
    assert L.modsx_describe_regions_dspsift(h, img, None, n, mr, 41, 0, 1, *dsp, p(buf)) == -1
    assert L.modsx_describe_regions_dspsift(h, img, p(regs), n, mr, 41, 0, 1, *dsp, None) == -1
    assert L.modsx_describe_regions_dspsift(h, None, p(regs), n, mr, 41, 0, 1, *dsp, p(buf)) == -1
    assert L.modsx_describe_regions_dspsift_device(h, img, p(regs), n, mr, 41, 0, 1, *dsp, None) == -1
    assert L.modsx_sift_norm_rows(h, p(buf), -1, d(0.2), p(buf)) == -1
    assert L.modsx_sift_norm_rows(h, None, 1, d(0.2), p(buf)) == -1
    assert L.modsx_sift_norm_rows(h, p(buf), 1, d(0.2), None) == -1
    assert L.modsx_sift_norm_rows_device(h, None, 1, d(0.2), None) == -1
    src, sp = _dev(np.ones((2, 128), np.float32), 4)
    for bad in ((sp + 1, sp), (sp, sp + 2)):                                  # not 4-byte aligned
        assert L.modsx_sift_norm_rows_device(h, C.c_void_p(bad[0]), 1, d(0.2), C.c_void_p(bad[1])) == -1
    assert L.modsx_describe_regions_raw_device(h, img, p(regs), n, mr, 41, 0, 1, C.c_void_p(sp + 1)) == -1
    assert L.modsx_describe_regions_dspsift_device(h, img, p(regs), n, mr, 41, 0, 1, *dsp, C.c_void_p(sp + 2)) == -1
    assert L.modsx_dsp_counters(h, None, 3) == -1
    same_bits(_back(src, 4, (2, 128)), np.ones((2, 128), np.float32), "a refused call writes nothing")
    # n == 0 succeeds and writes nothing
    assert ctx.sift_norm_rows(np.zeros((0, 128), np.float32)).shape == (0, 128)
    assert ctx.describe_regions_raw(image, regs[:0]).shape == (0, 128)
    assert ctx.describe_regions_dspsift(image, regs[:0]).shape == (0, 128)
    assert (ctx.dsp_counters(), ctx.describe_counters()) == before             # a refusal launches nothing
    cfg = Cs.CONFIGS[1]
    same_bits(ctx.describe_regions_dspsift(image, regs, mr_size=DC.MR_SIZE, num_scales=cfg[0], start_coef=cfg[1], end_coef=cfg[2]),
              dsp_ref[cfg], "after the refusals")
