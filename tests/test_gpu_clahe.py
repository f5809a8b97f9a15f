"""GPU: CLAHE on the device (the drivers' doCLAHE step: cv::CLAHE, OpenCV 2.4.9, and the 3.x / 4.x rule as variant 1) against
tests/clahe_model.py, stage by stage.

Comparison rule, everywhere: exact equality.  Through Context.debug_clahe the histograms of every tile before clipping and the
finished LUTs equal the model's byte for byte; through Context.clahe every output pixel equals the model's.  No tolerance: the
histograms, the clipping and the prefix sums are integers, the two f32 stages repeat the contract's operations in its order.

The cases are those of tests/clahe_cases.py; tests/test_clahe_cases_cpu.py proves without a device what they reach.
  1. histograms, LUTs and output of every case; in place equals out of place
  2. wrapped device memory at every 4-byte alignment (the scalar path of both pixel kernels)
  3. the mixed-size batch against the single calls, in place and out of place, and its counters
  4. a 3-channel upload; the detect -> orient -> describe chain on the small pair
  5. refusals; an unrelated describe_regions result before and after
"""
import numpy as np
import pytest

from tests import clahe_cases as CC
from tests import clahe_model as M
from tests.common import same_records

pytestmark = pytest.mark.gpu


def _par(c):
    return dict(clip_limit=c["clip"], tiles=c["grid"], variant=c["variant"])


def _first_diff(got, ref):
    bad = np.argwhere(got != ref)
    return None if not len(bad) else (len(bad), tuple(int(v) for v in bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


def _check_case(ctx, k, img=None):
    """the three stages of case k on the device against the model; img: an Image that already holds the case's pixels"""
    c, e = CC.CASES[k], CC.expected(k)
    own = img is None
    if own:
        img = ctx.upload(CC.image(k))
    try:
        dbg = ctx.debug_clahe(img, **_par(c))
        assert _first_diff(dbg["hist"], e["hist"]) is None, (CC.name(k), "histogram (count, tile/bin, got, model)", _first_diff(dbg["hist"], e["hist"]))
        assert _first_diff(dbg["lut"], e["lut"]) is None, (CC.name(k), "LUT (count, tile/value, got, model)", _first_diff(dbg["lut"], e["lut"]))
        out = ctx.clahe(img, **_par(c))
        got = out.download()
        out.free()
        ref = e["out"].astype(np.float32)
        assert got.shape == ref.shape
        assert _first_diff(got, ref) is None, (CC.name(k), "output (count, y/x, got, model)", _first_diff(got, ref))
        return got
    finally:
        if own:
            img.free()


# ------------------------------------------------------------------------------------------------------------ 1. every case
@pytest.mark.parametrize("lo", range(0, len(CC.SMALL), 32))
def test_small_cases_stage_by_stage(ctx, lo):
    for k in CC.SMALL[lo:lo + 32]:
        _check_case(ctx, k)


@pytest.mark.parametrize("k", [k for k in range(len(CC.CASES)) if k not in CC.SMALL], ids=CC.name)
def test_big_cases_stage_by_stage(ctx, k):
    _check_case(ctx, k)


def test_in_place_equals_out_of_place(ctx):
    picks = [k for k in CC.SMALL if CC.CASES[k]["shape"] in ((9, 17), (135, 239), CC.TWO_STRIPS)][::3] + [CC.BATCH[-1]]
    for k in picks:
        c = CC.CASES[k]
        img = ctx.upload(CC.image(k))
        assert ctx.clahe(img, out=img, **_par(c)) is img
        got = img.download()
        img.free()
        assert np.array_equal(got, CC.expected(k)["out"].astype(np.float32)), CC.name(k)


# ------------------------------------------------------------------------------------------------------------ 2. alignment
def _dev(pixels, offset):
    """f32 values in a torch buffer on the device, `offset` bytes into it: (keep-alive, device pointer)"""
    import torch
    pixels = np.ascontiguousarray(pixels, np.float32)
    buf = torch.zeros(pixels.size * 4 + 64, dtype=torch.uint8, device="cuda")
    buf[offset:offset + pixels.size * 4] = torch.from_numpy(pixels.reshape(-1).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _back(buf, offset, shape):
    import torch
    torch.cuda.synchronize()
    n = int(np.prod(shape)) * 4
    return buf[offset:offset + n].cpu().numpy().view(np.float32).reshape(shape).copy()


@pytest.mark.parametrize("offset", [0, 4, 8, 12])
def test_wrapped_memory_at_every_alignment(ctx, offset):
    for k in [k for k in CC.SMALL if CC.CASES[k]["shape"] in ((9, 17), (131, 257)) and CC.CASES[k]["kind"] in ("noise", "f32_edges")][:6]:
        c, e = CC.CASES[k], CC.expected(k)
        rows, cols = c["shape"]
        src, psrc = _dev(CC.image(k), offset)
        dst, pdst = _dev(np.full(c["shape"], -1.0, np.float32), (offset + 8) % 16)
        a, b = ctx.wrap_device(psrc, rows, cols), ctx.wrap_device(pdst, rows, cols)
        try:
            _check_case(ctx, k, img=a)
            ctx.clahe(a, out=b, **_par(c))
            assert np.array_equal(_back(dst, (offset + 8) % 16, c["shape"]), e["out"].astype(np.float32)), (CC.name(k), offset)
            assert _back(src, offset, c["shape"]).tobytes() == CC.image(k).tobytes()          # the source is left as it was
            guard = dst.cpu().numpy()
            assert not guard[:(offset + 8) % 16].any() and not guard[(offset + 8) % 16 + rows * cols * 4:].any()   # nothing written beside it
        finally:
            a.free(); b.free()


# ------------------------------------------------------------------------------------------------------------ 3. the batch
def test_batch_of_mixed_sizes_equals_single_calls(ctx, modsx):
    ks = CC.BATCH
    imgs = [ctx.upload(CC.image(k)) for k in ks]
    outs = [ctx.upload(np.zeros(CC.CASES[k]["shape"], np.float32)) for k in ks]
    try:
        before = ctx.clahe_counters()
        assert ctx.clahe_batch(imgs, out=outs) == outs
        after = ctx.clahe_counters()
        geos = [modsx.clahe_geometry(*CC.CASES[k]["shape"]) for k in ks]
        delta = {f: after[f] - before[f] for f in after}
        assert delta == dict(calls=1, images=len(ks), tiles=64 * len(ks), strips=64 * sum(g["strips"] for g in geos),
                             pixels=sum(CC.image(k).size for k in ks), launches=3)               # one launch set for all of them
        for k, im, o in zip(ks, imgs, outs):
            single = ctx.clahe(im)
            want = single.download()
            single.free()
            assert np.array_equal(want, CC.expected(k)["out"].astype(np.float32)), CC.name(k)
            assert o.download().tobytes() == want.tobytes(), CC.name(k)
            assert im.download().tobytes() == CC.image(k).tobytes()
        ctx.clahe_batch(imgs)                                                                      # in place
        for k, im, o in zip(ks, imgs, outs):
            assert im.download().tobytes() == o.download().tobytes(), CC.name(k)
        assert ctx.clahe_batch([]) == []
    finally:
        for im in imgs + outs:
            im.free()


def test_batch_with_other_parameters(ctx):
    ks = [k for k in CC.SMALL if CC.CASES[k]["grid"] == (3, 5) and CC.CASES[k]["variant"] == 1 and CC.CASES[k]["clip"] == 4.0
          and CC.CASES[k]["kind"] == "noise"]
    assert len(ks) >= 6
    imgs = [ctx.upload(CC.image(k)) for k in ks]
    try:
        ctx.clahe_batch(imgs, tiles=(3, 5), variant=1)
        for k, im in zip(ks, imgs):
            assert np.array_equal(im.download(), CC.expected(k)["out"].astype(np.float32)), CC.name(k)
    finally:
        for im in imgs:
            im.free()


# ------------------------------------------------------------------------------------------------------------ 4. around it
def test_three_channel_upload(ctx):
    bgr = np.random.RandomState(77).randint(0, 256, (100, 75, 3)).astype(np.uint8)
    img = ctx.upload(bgr)
    gray = img.download()                                 # (B + G + R) / 3 as the upload made it
    e = M.run(gray)
    assert (gray != np.rint(gray)).any()                  # thirds: the conversion to bytes rounds here
    out = ctx.clahe(img)
    got = out.download()
    img.free(); out.free()
    assert np.array_equal(got, e["out"].astype(np.float32))


def _chain(ctx, modsx, img):
    kps = ctx.detect_affine_keypoints(img, modsx.default_hessaff_params())
    regs = ctx.detect_orientation(img, modsx.detect_affine_regions(kps))
    return kps, regs, ctx.describe_regions(img, regs)


def test_chain_after_clahe_equals_chain_on_the_models_output(ctx, modsx, small_pair):
    for pixels in small_pair[:2]:
        pixels = np.ascontiguousarray(pixels, np.float32)
        src = ctx.upload(pixels)
        eq = ctx.clahe(src)
        ref = ctx.upload(M.run(pixels)["out"].astype(np.float32))
        try:
            got, want = _chain(ctx, modsx, eq), _chain(ctx, modsx, ref)
            assert len(got[0]) > 50
            assert same_records(got[0], want[0]) and same_records(got[1], want[1])
            assert got[2].tobytes() == want[2].tobytes()
            plain = ctx.detect_affine_keypoints(src, modsx.default_hessaff_params())
            assert not same_records(plain, got[0])        # the equalised image is another image
        finally:
            src.free(); eq.free(); ref.free()


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_launch_nothing(ctx, modsx):
    a = ctx.upload(CC.image(CC.BATCH[3]))
    b = ctx.upload(np.zeros((64, 65), np.float32))
    c = ctx.upload(CC.image(CC.BATCH[3]))
    host = np.zeros((64, 64), np.float32)
    w = ctx.wrap_device(host.ctypes.data, 64, 64)
    before = ctx.clahe_counters()
    try:
        for kw, word in [(dict(tiles=(0, 8)), "tiles"), (dict(tiles=(8, 0)), "tiles"), (dict(tiles=(17, 16)), "256"), (dict(clip_limit=-1.0), "clip_limit"),
                         (dict(clip_limit=float("nan")), "clip_limit"), (dict(clip_limit=float("inf")), "clip_limit"), (dict(variant=2), "variant")]:
            for call in (lambda: ctx.clahe(a, **kw), lambda: ctx.clahe(a, out=c, **kw), lambda: ctx.clahe_batch([a], **kw), lambda: ctx.debug_clahe(a, **kw)):
                with pytest.raises(RuntimeError, match=word):
                    call()
        with pytest.raises(RuntimeError, match="another size"):
            ctx.clahe(a, out=b)
        with pytest.raises(RuntimeError, match="another size"):
            ctx.clahe_batch([a, a], out=[c, b])
        with pytest.raises(RuntimeError, match="device memory"):
            ctx.clahe(w)
        with pytest.raises(RuntimeError, match="device memory"):
            ctx.clahe(a, out=w)
        with pytest.raises(RuntimeError, match="share their pixels"):
            ctx.clahe_batch([a, c], out=[c, c])
        with pytest.raises(RuntimeError, match="another image's input"):
            ctx.clahe_batch([a, c], out=[c, a])
        assert ctx.clahe_counters() == before                       # nothing was launched or booked
        assert a.download().tobytes() == CC.image(CC.BATCH[3]).tobytes() and not b.download().any()
        assert c.download().tobytes() == CC.image(CC.BATCH[3]).tobytes()
        out = ctx.clahe(a, tiles=(16, 16))                          # 256 tiles: the limit itself works
        assert np.array_equal(out.download(), M.run(CC.image(CC.BATCH[3]), 4.0, (16, 16))["out"].astype(np.float32))
        out.free()
        import torch
        # last in the test: freeing on the other device makes it the thread's current one until the frees below go through ctx again
        if torch.cuda.device_count() > 1:
            before = ctx.clahe_counters()
            other = modsx.Context(1)
            far = other.upload(CC.image(CC.BATCH[3]))
            try:
                with pytest.raises(RuntimeError, match="another device"):
                    ctx.clahe(far)
                with pytest.raises(RuntimeError, match="another device"):
                    ctx.clahe(a, out=far)
                assert ctx.clahe_counters() == before
            finally:
                far.free(); other.close()
    finally:
        for im in (a, b, c, w):
            im.free()


def test_unrelated_describe_result_is_unchanged_around_clahe_calls(ctx, modsx, small_pair):
    img = ctx.upload(np.ascontiguousarray(small_pair[0], np.float32))
    try:
        first = _chain(ctx, modsx, img)
        k = CC.BATCH[-1]
        big = ctx.upload(CC.image(k))
        ctx.clahe(big, out=big)
        ctx.debug_clahe(big, tiles=(16, 16))
        big.free()
        again = ctx.describe_regions(img, first[1])
        assert again.tobytes() == first[2].tobytes()
        assert same_records(ctx.detect_affine_keypoints(img, modsx.default_hessaff_params()), first[0])
    finally:
        img.free()
