"""GPU: the learned-descriptor front end, bit for bit (f32 as uint32, NaN by position) against tests/caffe_model.py -- the
restatement that tests/test_caffe_model_cpu.py ties to the compiled interpolate and to the recorded norms of the reference.  The
inputs are those of tests/caffe_cases.py.
  1. caffe_patches on every (image, colour or gray, patch size, mean), from the host and into a device pointer 4 bytes off; flags
     and counters; every region count at patch sizes 41 and 65; two calls equal one
  2. caffe_norm_rows at every width and norm against the model and the fixture: from the host, in place on device rows 4 bytes off
  3. rep_append_f32_device against the host append
  4. the chain detect -> orient -> reproject -> describe_learned -> rep_append_f32_device -> rep_match_fginn_f32
  5. the refusals through the binding

Fault latch: a HIP error met by any test of this module sets _FAULT; every later test then fails at once, before it touches the
GPU -- nothing is retried."""
import ctypes as C
import os

import numpy as np
import pytest

import caffe_cases as Cs
import caffe_model as M
import fginn32_cases as FC
from common import same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "hipmemcpy", "hipstream",
                   "hipgetlasterror", "unspecified launch failure", "queue error")
_FAULT = None


class _Gpu(object):
    """the body of a test: a device error inside it ends the module's GPU work"""

    def __enter__(self):
        if _FAULT is not None:
            pytest.fail("an earlier test of this module met a device error; nothing more is started on the GPU:\n%s" % _FAULT, pytrace=False)

    def __exit__(self, et, ev, tb):
        global _FAULT
        if ev is not None and isinstance(ev, RuntimeError) and any(m in str(ev).lower() for m in HIP_ERROR_MARKS):
            _FAULT = str(ev)[-1500:]
        return False


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not got.size:
        return
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN entries differ in rows", list(np.nonzero((np.isnan(got) != nan).reshape(len(got), -1).any(1))[0][:10]))
    bad = np.nonzero(((u32(got) != u32(ref)) & ~nan).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, (what, "rows that differ:", list(bad[:10]), len(bad))


def _dev(values, offset):
    """f32 values in a torch buffer on the device, `offset` bytes into it: (keep-alive, device pointer)"""
    import torch
    values = np.ascontiguousarray(values, np.float32)
    buf = torch.zeros(values.size * 4 + 64, dtype=torch.uint8, device="cuda")
    if values.size:
        buf[offset:offset + values.size * 4] = torch.from_numpy(values.reshape(-1).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _back(buf, offset, shape):
    import torch
    torch.cuda.synchronize()
    n = int(np.prod(shape)) * 4
    return buf[offset:offset + n].cpu().numpy().view(np.float32).reshape(shape).copy()


def _untouched(buf, offset, floats):
    return not buf[:offset].cpu().numpy().any() and not buf[offset + floats * 4:].cpu().numpy().any()


@pytest.fixture(scope="module")
def uploaded(ctx):
    """{image: {True: [B, G, R handles], False: [gray handle]}}"""
    imgs = {name: {True: [ctx.upload(p) for p in Cs.planes(name)], False: [ctx.upload(Cs.gray(name))]} for name in Cs.IMAGES}
    yield imgs
    for d in imgs.values():
        for hs in d.values():
            for h in hs:
                h.free()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "caffe_norm_ref.npz"))


# ----------------------------------------------------------------------------------------------------------- caffe_patches
@pytest.mark.parametrize("P", Cs.PATCH_SIZES)
def test_patches_flags_and_counters_against_the_model(ctx, modsx, uploaded, P):
    with _Gpu():
        for name in Cs.IMAGES:
            regs = Cs.regions(name, P)
            counts = (len(regs),) + (Cs.COUNTS if P in Cs.ALL_COUNTS_AT else ())
            for colour in (True, False):
                b, border, outside = Cs.model_bytes(name, colour, P)
                planes = uploaded[name][colour]
                for mean in Cs.MEANS:
                    par = modsx.caffe_params(patch_size=P, mean=mean)
                    for n in counts:
                        idx = np.arange(n) % len(regs)
                        what = "%s, %s, P = %d, mean %r, n = %d" % (name, "colour" if colour else "gray", P, mean, n)
                        want, wflags = M.blob(b[idx], mean), M.flags(border[idx], outside[idx])
                        before = ctx.caffe_counters()
                        got, fl = ctx.caffe_patches(planes, regs[idx], par, want_flags=True)
                        d = {k: v - before[k] for k, v in ctx.caffe_counters().items()}
                        same_bits(got, want, what)
                        assert np.array_equal(fl, wflags), (what, fl, wflags)
                        assert d == (dict(calls=1, regions=n, border_regions=int(border[idx].sum()), launches=1) if n else
                                     dict(calls=0, regions=0, border_regions=0, launches=0)), (what, d)
                        dst, dp = _dev(np.zeros(want.shape, np.float32), 4)
                        assert dp % 8 == 4
                        blob, fl = ctx.caffe_patches(planes, regs[idx], par, out_ptr=dp, want_flags=True)
                        assert blob is None and np.array_equal(fl, wflags), what
                        same_bits(_back(dst, 4, want.shape), want, what + ", device blob")
                        assert _untouched(dst, 4, want.size), what                      # nothing written outside the n patches
                    if tuple(mean) == (0.0, 0.0, 0.0):                                   # the raw bytes
                        assert np.array_equal(ctx.caffe_patches(planes, regs, par), b.astype(np.float32))
                k = Cs.REGION_NAMES.index("outside")
                par = modsx.caffe_params(patch_size=P, mean=Cs.MEANS[1])
                assert (ctx.caffe_patches(planes, regs[k:k + 1], par)[0] == np.array([-104.0, 3.0, 0.0], np.float32)[:, None, None]).all()


@pytest.mark.parametrize("P", (41, 129))
def test_two_calls_equal_one(ctx, modsx, uploaded, P):
    with _Gpu():
        regs = Cs.take(Cs.regions("a", P), 65)
        par = modsx.caffe_params(patch_size=P)
        for colour in (True, False):
            one, f1 = ctx.caffe_patches(uploaded["a"][colour], regs, par, want_flags=True)
            for cut in (1, 23, 64):
                a, fa = ctx.caffe_patches(uploaded["a"][colour], regs[:cut], par, want_flags=True)
                b, fb = ctx.caffe_patches(uploaded["a"][colour], regs[cut:], par, want_flags=True)
                assert np.concatenate([a, b]).tobytes() == one.tobytes() and np.array_equal(np.concatenate([fa, fb]), f1), (P, colour, cut)


def test_flags_may_be_left_out_and_only_reproj_kp_is_read(ctx, modsx, uploaded):
    with _Gpu():
        regs = Cs.regions("b", 41)
        par = modsx.caffe_params()
        want = ctx.caffe_patches(uploaded["b"][True], regs, par)
        other = regs.copy()
        other["det_kp"]["x"], other["det_kp"]["s"], other["img_id"], other["id"] = -5.0, 0.0, 9, 77
        assert ctx.caffe_patches(uploaded["b"][True], other, par).tobytes() == want.tobytes()
        same_bits(want, M.blob(Cs.model_bytes("b", True, 41)[0], Cs.MEANS[0]))


# --------------------------------------------------------------------------------------------------------- caffe_norm_rows
@pytest.mark.parametrize("w", Cs.NORM_WIDTHS)
def test_norm_rows_against_the_model_and_the_fixture(ctx, modsx, golden, w):
    with _Gpu():
        base = Cs.norm_rows(w)
        for norm in Cs.NORMS + (M.NORM_NONE,):
            if norm != M.NORM_NONE:
                same_bits(ctx.caffe_norm_rows(base, norm), golden["%s_%d" % (Cs.NORM_NAMES[norm], w)], "fixture, norm %d, width %d" % (norm, w))
            for n in Cs.NORM_ROW_COUNTS:
                what = "norm %d, width %d, %d rows" % (norm, w, n)
                rows = Cs.take_rows(w, n)
                want = M.norm_rows(rows, norm)
                same_bits(ctx.caffe_norm_rows(rows, norm), want, what)
                buf, p = _dev(rows, 4)
                assert p % 8 == 4
                ctx.caffe_norm_rows_device(p, n, w, norm)                      # in place
                same_bits(_back(buf, 4, rows.shape), want, what + ", in place on the device")
                assert _untouched(buf, 4, rows.size), what
        rows = Cs.take_rows(w, 65)
        src, sp = _dev(rows, 4)
        dst, dp = _dev(np.zeros(rows.shape, np.float32), 0)
        ctx.caffe_norm_rows_device(sp, 65, w, M.NORM_ROOTL2, out_ptr=dp)            # out of place: the source is left as it was
        same_bits(_back(dst, 0, rows.shape), M.norm_rows(rows, M.NORM_ROOTL2), "out of place")
        assert _back(src, 4, rows.shape).tobytes() == rows.tobytes()


# --------------------------------------------------------------------------------------------------- rep_append_f32_device
def _rows(n, dim, seed):
    return (np.random.RandomState(seed).standard_normal((n, dim)) * 40.0).astype(np.float32)


def test_device_append_equals_the_host_append(ctx, modsx):
    with _Gpu():
        HES, CAFFE = modsx.DET_HESSIAN, modsx.DESC_CAFFE
        for dim in (4, 128, 256):
            regs = Cs.take(Cs.regions("a", 41), 70)
            regs["id"] = np.arange(70)
            rows = _rows(70, dim, dim)
            host, dev = modsx.Rep(ctx), modsx.Rep(ctx)
            try:
                for a, b in ((0, 41), (41, 41), (41, 70)):                      # a second append behind the first; an empty one
                    buf, p = _dev(rows[a:b], 4)
                    assert host.append_f32(regs[a:b], rows[a:b], HES, CAFFE) == b - a
                    assert dev.append_f32_device(regs[a:b], p, dim, HES, CAFFE) == b - a
                    assert dev.count_f32(HES, CAFFE) == host.count_f32(HES, CAFFE) == b
                (hr, hd), (dr, dd) = host.class_f32(HES, CAFFE), dev.class_f32(HES, CAFFE)
                assert dd.shape == (70, dim) and dd.tobytes() == hd.tobytes() == rows.tobytes()
                assert same_records(dr, hr) and same_records(dr, regs)
                q = modsx.Rep(ctx)
                q.append_f32(regs[:30], _rows(30, dim, 5), HES, CAFFE)
                FC.same_tents(ctx.rep_match_fginn_f32(q, dev, HES, CAFFE), ctx.rep_match_fginn_f32(q, host, HES, CAFFE))
                q.free()
            finally:
                host.free(); dev.free()


def test_device_append_refuses_what_the_host_append_refuses(ctx, modsx):
    with _Gpu():
        L, HES, CAFFE = modsx.lib(), modsx.DET_HESSIAN, modsx.DESC_CAFFE
        regs = Cs.take(Cs.regions("a", 41), 8)
        rows = _rows(8, 128, 1)
        buf, p = _dev(rows, 4)
        rp = regs.ctypes.data_as(C.c_void_p)
        rep = modsx.Rep(ctx)
        try:
            assert rep.append_f32_device(regs, p, 128, HES, CAFFE) == 8
            bad = rows.copy(); bad[5, 77] = np.nan
            huge = rows.copy(); huge[0, 0] = 2e17
            for r in (bad, huge):
                b2, p2 = _dev(r, 4)
                with pytest.raises(RuntimeError, match="finite"):
                    rep.append_f32_device(regs, p2, 128, HES, CAFFE)
                with pytest.raises(RuntimeError, match="finite"):
                    rep.append_f32(regs, r, HES, CAFFE)
            for call in (lambda: rep.append_f32_device(regs, p, 64, HES, CAFFE), lambda: rep.append_f32(regs, rows[:, :64], HES, CAFFE)):
                with pytest.raises(RuntimeError, match="another width"):
                    call()
            for det, typ, dim in ((HES, modsx.DESC_SURF, 128), (HES, modsx.DESC_LIOP, 128), (modsx.DET_MSER, CAFFE, 126), (HES, CAFFE, 0),
                                  (HES, CAFFE, 260)):
                with pytest.raises(RuntimeError, match="width"):
                    rep.append_f32_device(regs, p, dim, det, typ)
            for det, typ in ((modsx.DET_ORB, CAFFE), (HES, 1), (HES, 13), (HES, modsx.DESC_ORB)):
                with pytest.raises(RuntimeError, match="bad argument"):
                    rep.append_f32_device(regs, p, 128, det, typ)
                with pytest.raises(RuntimeError, match="bad argument"):
                    rep.append_f32(regs, rows, det, typ)
            h, r = ctx._c(), C.c_void_p(rep.h)
            for fn in (L.modsx_rep_append_f32_device, L.modsx_rep_append_f32):
                src = C.c_void_p(p) if fn is L.modsx_rep_append_f32_device else rows.ctypes.data_as(C.c_void_p)
                assert fn(h, r, HES, CAFFE, rp, src, 128, -1) == -1
                assert fn(h, r, HES, CAFFE, None, src, 128, 8) == -1
                assert fn(h, r, HES, CAFFE, rp, None, 128, 8) == -1
                assert fn(h, None, HES, CAFFE, rp, src, 128, 8) == -1
                assert fn(None, r, HES, CAFFE, rp, src, 128, 8) == -1
                assert fn(h, r, HES, CAFFE, rp, src, 128, 2000001) == -1 and b"2 000 000" in L.modsx_last_error()
            assert L.modsx_rep_append_f32_device(h, r, HES, CAFFE, rp, C.c_void_p(p + 2), 128, 8) == -1          # not 4-byte aligned
            # the class is what the one good append left
            gr, gd = rep.class_f32(HES, CAFFE)
            assert gd.tobytes() == rows.tobytes() and same_records(gr, regs)
            assert rep.append_f32_device(regs[:3], p, 128, HES, CAFFE) == 3 and rep.count_f32(HES, CAFFE) == 11
        finally:
            rep.free()


# ------------------------------------------------------------------------------------------------------------------- chain
def test_chain_on_small_pair(ctx, modsx, oracle, small_pair):
    """detect -> orient -> reproject -> describe_learned -> rep_append_f32_device -> rep_match_fginn_f32 against the oracle's
    match_fginn on the model's rows.  The network is an exact stand-in: a strided slice of the blob, no arithmetic."""
    import torch
    from mods_amd.learned import describe_learned
    with _Gpu():
        a, b, _ = small_pair
        par = modsx.caffe_params()
        pick = lambda blob: blob.reshape(blob.shape[0], -1)[:, ::39][:, :128]      # noqa: E731
        HES, CAFFE = modsx.DET_HESSIAN, modsx.DESC_CAFFE
        reps, sides = [], []
        try:
            for g in (a, b):
                g = np.ascontiguousarray(g, np.float32)
                im = ctx.upload(g)
                try:
                    k = ctx.detect_affine_keypoints(im, modsx.default_hessaff_params())
                    ro = ctx.detect_orientation(im, modsx.detect_affine_regions(k))
                    regs = modsx.reproject_regions(ro, np.eye(3), g.shape[1], g.shape[0])
                    rows = describe_learned(ctx, [im], regs, pick, par, "L2", batch=100)
                finally:
                    im.free()
                assert len(regs) > 100 and rows.shape == (len(regs), 128) and rows.dtype == torch.float32 and rows.is_contiguous()
                want = M.norm_rows(pick(M.blob(M.patch_bytes((g,), regs, par.mrSize, 41)[0], Cs.MEANS[0])), M.NORM_L2)
                assert np.isfinite(want).all()
                same_bits(rows.cpu().numpy(), want, "describe_learned")
                rep = modsx.Rep(ctx)
                reps.append(rep)
                assert rep.append_f32_device(regs, rows.data_ptr(), 128, HES, CAFFE) == len(regs)
                sides.append((regs, want))
            mp = modsx.default_pair_params()
            got = ctx.rep_match_fginn_f32(reps[0], reps[1], HES, CAFFE, mp.match_ratio, mp.contradDist, mp.nn)
            (r1, m1), (r2, m2) = sides
            pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
            tent = oracle.match_fginn(m1, m2, pos2, mp.match_ratio, mp.contradDist, mp.nn)
            assert len(tent) > 0, "a chain without a tentative compares empty lists"
            FC.same_tents(got, tent)
        finally:
            for r in reps:
                r.free()


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(ctx, modsx, uploaded):
    with _Gpu():
        regs = Cs.regions("a", 41)
        col, gry = uploaded["a"][True], uploaded["a"][False]
        before = ctx.caffe_counters()
        for ps in (0, 2, 40, 256):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+patchSize"):
                ctx.caffe_patches(col, regs, modsx.caffe_params(patch_size=ps))
        for mr in (float("nan"), -1.0, 2e6):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+mrSize"):
                ctx.caffe_patches(col, regs, modsx.caffe_params(mr_size=mr))
        with pytest.raises(RuntimeError, match=r"\(-1\): .+mean"):
            ctx.caffe_patches(col, regs, modsx.caffe_params(mean=(0, float("inf"), 0)))
        for planes in (col[:2], col + gry, []):
            with pytest.raises(RuntimeError, match=r"\(-1\): .+planes"):
                ctx.caffe_patches(planes, regs)
        with pytest.raises(RuntimeError, match="different sizes"):
            ctx.caffe_patches([col[0], uploaded["b"][True][1], col[2]], regs)
        host = np.zeros((48, 64), np.float32)
        w = ctx.wrap_device(host.ctypes.data, 48, 64)
        try:
            with pytest.raises(RuntimeError, match="device memory"):
                ctx.caffe_patches([col[0], w, col[2]], regs)
            with pytest.raises(RuntimeError, match="device memory"):
                ctx.caffe_patches([col[0], w, col[2]], regs[:0])               # also with nothing to do
        finally:
            w.free()
        buf, p = _dev(np.zeros(len(regs) * 3 * 41 * 41, np.float32), 4)
        with pytest.raises(RuntimeError, match="aligned"):
            ctx.caffe_patches(col, regs, out_ptr=p + 2)
        rows = Cs.take_rows(64, 3)
        with pytest.raises(RuntimeError, match="norm"):
            ctx.caffe_norm_rows(rows, 4)
        with pytest.raises(RuntimeError, match="dim"):
            ctx.caffe_norm_rows(np.zeros((1, 4097), np.float32), 0)
        with pytest.raises(RuntimeError, match="bad argument"):
            ctx.caffe_norm_rows_device(p + 1, 3, 64, 0)
        assert ctx.caffe_counters() == before                                  # a refusal launches nothing
        assert _untouched(buf, 4, len(regs) * 3 * 41 * 41) and not _back(buf, 4, (len(regs) * 3 * 41 * 41,)).any()
        # n == 0 succeeds and writes nothing
        assert ctx.caffe_patches(col, regs[:0]).shape == (0, 3, 41, 41)
        assert ctx.caffe_patches(col, regs[:0], out_ptr=p) is None
        assert ctx.caffe_norm_rows(np.zeros((0, 64), np.float32), 0).shape == (0, 64)
        ctx.caffe_norm_rows_device(p, 0, 64, 0)
        assert ctx.caffe_counters() == before and not _back(buf, 4, (64,)).any()
        same_bits(ctx.caffe_patches(col, regs), M.blob(Cs.model_bytes("a", True, 41)[0], Cs.MEANS[0]), "after the refusals")
