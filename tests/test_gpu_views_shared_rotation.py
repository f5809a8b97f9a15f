"""GPU: views of one launch set that share a rotation are rotated once per tile (k_views_fused for a group of views,
mods_amd/csrc/kernels_views.hip; the grouping rule: tests/test_views_groups_cpu.py).

Every comparison is np.array_equal: against oracle.synth_view (same operations on the same operands in the same order), against
the same view synthesised alone through Context.synth_view (a group of one), and, for the switch MODSX_VIEWS_SHARE_ROT=0, against a
child process.  The view counters say that the views under test were in fact grouped.  The images are small random f32 ones whose
rotated sizes are no multiples of the 128 x 16 tile."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import views_share_child as CH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "views_share_child.py")
CHILD_TIMEOUT_S = 120          # import + context creation + one call; what tests/test_gpu_daisy.py allows such a child
SIZES = ((80, 96), (150, 203))           # rows, cols


def _image(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((rows, cols)) * 255.0).astype(np.float32)


@pytest.fixture(scope="module")
def images(ctx):
    out = {}
    for k, (rows, cols) in enumerate(SIZES):
        a = _image(rows, cols, 41 + k)
        out[(rows, cols)] = (a, ctx.upload(a))
    yield out
    for _, im in out.values():
        im.free()


def _oracle_views(oracle, a, args_list):
    return [oracle.synth_view(a, oracle.make_view(*args)) for args in args_list]


def _args(views):
    return [(v.tilt, v.phi, v.zoom, v.InitSigma, v.doBlur) for v in views]


def _run_set(ctx, modsx, items):
    """items: [(Image, view)] as ONE launch set -> ([pixels or None for an identity view], (views fused, groups, rotated pixels))"""
    modsx.views_counters(reset=True)
    got = ctx.synth_views([im for im, _ in items], [v for _, v in items])
    counters = modsx.views_counters(reset=True)
    out = []
    for g, ident in got:
        out.append(None if ident else g.download())
        g.free()
    return out, counters


def _same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), (what, int((got != ref).sum()), np.argwhere(got != ref)[:4].tolist())


def _check_set(ctx, modsx, oracle, a, im, views, alone=True):
    got, counters = _run_set(ctx, modsx, [(im, v) for v in views])
    refs = _oracle_views(oracle, a, _args(views))
    for v, g, (ref, _, ident) in zip(views, got, refs):
        what = (a.shape, v.tilt, v.phi, v.zoom, v.InitSigma)
        assert (g is None) == bool(ident), what
        if ident:
            continue
        _same(g, ref, what)
        if alone:
            one, _, _ = ctx.synth_view(im, v)
            try:
                _same(one.download(), g, ("alone",) + what)
            finally:
                one.free()
    return counters


@pytest.mark.parametrize("size", SIZES)
def test_headline_ladder_in_one_launch_set(ctx, modsx, oracle, images, size):
    """The 31 views of the headline at InitSigma 0.2: 30 fused views in 18 groups, every view the oracle's and the one the
    single-view entry makes."""
    a, im = images[size]
    views = modsx.set_vs_pars(*CH.HEADLINE, [])
    assert len(views) == 31
    plans = [p for p in (modsx.view_plan(size[0], size[1], v) for v in views) if not p["identity"]]
    assert any(p["w_rot"] % 128 and p["h_rot"] % 16 for p in plans)
    want = modsx.views_groups(plans)
    assert (want["views_fused"], want["groups"]) == (30, 18)
    counters = _check_set(ctx, modsx, oracle, a, im, views)
    assert counters == (30, 18, want["rotated_pixels"]), counters
    assert want["rotated_pixels"] < want["rotated_pixels_alone"]


@pytest.mark.parametrize("size", SIZES)
def test_members_of_a_group_differ_in_both_filter_widths(ctx, modsx, oracle, images, size):
    """ScaleSet [1, 0.25], tilts 2 and 4, InitSigma 0.5: all 18 views stay on the fused launch, and the four views of an angle
    have 5, 7, 13 and 25 taps along x and 3 and 5 along y, so a group's halo is wider than most of its members' in x and in y."""
    a, im = images[size]
    views = modsx.set_vs_pars([1.0, 0.25], [2, 4], 120.0, 0.5, 1, [])
    plans = [modsx.view_plan(size[0], size[1], v) for v in views]
    assert len(views) == 18 and all(p["kind"] == 2 and not p["identity"] for p in plans)
    want = modsx.views_groups(plans)
    assert (want["views_fused"], want["groups"]) == (18, 6)
    mixed = 0
    for k in range(want["groups"]):
        kx = {p["kx"] for p, gk in zip(plans, want["group"]) if gk == k}
        ky = {p["ky"] for p, gk in zip(plans, want["group"]) if gk == k}
        mixed += len(kx) > 1 and len(ky) > 1
    assert mixed == 6, "every group mixes filter widths in x and in y"
    counters = _check_set(ctx, modsx, oracle, a, im, views)
    assert counters == (18, 6, want["rotated_pixels"]), counters


def test_a_view_off_the_fused_kernel_leaves_its_partners_grouped(ctx, modsx, oracle, images):
    """Zoom 0.125 at InitSigma 0.5 filters 7 rows: beyond the tile's halo, so that view takes the separate launches; a view
    without a blur does too.  Their partners of the same angle are grouped, and all four are exact."""
    size = SIZES[1]
    a, im = images[size]
    phi = math.pi / 3
    views = [modsx.make_view(2.0, phi, 1.0, 0.5, 1), modsx.make_view(2.0, phi, 0.125, 0.5, 1), modsx.make_view(4.0, phi, 1.0, 0.5, 1),
             modsx.make_view(4.0, phi, 1.0, 0.5, 0)]
    plans = [modsx.view_plan(size[0], size[1], v) for v in views]
    assert [p["kind"] for p in plans] == [2, 0, 2, 0]
    counters = _check_set(ctx, modsx, oracle, a, im, views)
    assert counters == (2, 1, plans[0]["w_rot"] * plans[0]["h_rot"]), counters


def test_rotated_image_narrower_than_a_tile(ctx, modsx, oracle):
    """40 x 30 and 96 x 80 sources: every rotated image is below 128 columns, some below 16 rows of the last tile row"""
    for rows, cols in ((30, 40), SIZES[0]):
        a = _image(rows, cols, 7)
        views = modsx.set_vs_pars([1.0], [1, 2, 4], 120.0, 0.2, 1, [])
        plans = [p for p in (modsx.view_plan(rows, cols, v) for v in views) if not p["identity"]]
        assert all(p["w_rot"] < 128 for p in plans) and len(plans) == 9
        im = ctx.upload(a)
        try:
            counters = _check_set(ctx, modsx, oracle, a, im, views)
        finally:
            im.free()
        assert counters[:2] == (9, 6), counters


def test_two_images_in_one_launch_set(ctx, modsx, oracle, images):
    """The views of two images interleaved in one set (as the view-sharded path batches them): a group never spans two images."""
    (a, ia), (b, ib) = images[SIZES[0]], images[SIZES[1]]
    views = [v for v in modsx.set_vs_pars([1.0], [1, 2, 4], 120.0, 0.2, 1, [])]
    items, srcs = [], []
    for v in views:
        items += [(ia, v), (ib, v)]
        srcs += [a, b]
    assert len(items) == 20
    got, counters = _run_set(ctx, modsx, items)
    rot = 0
    for (rows, cols) in SIZES:
        plans = [p for p in (modsx.view_plan(rows, cols, v) for v in views) if not p["identity"]]
        rot += modsx.views_groups(plans)["rotated_pixels"]
    assert counters == (18, 12, rot), counters
    for (im, v), src, g in zip(items, srcs, got):
        ref, _, ident = oracle.synth_view(src, oracle.make_view(v.tilt, v.phi, v.zoom, v.InitSigma, v.doBlur))
        assert (g is None) == bool(ident)
        if not ident:
            _same(g, ref, (src.shape, v.tilt, v.phi))
    # the same image under two handles: equal pixels, another buffer, no common group
    ia2 = ctx.upload(a)
    try:
        _, counters = _run_set(ctx, modsx, [(ia, views[1]), (ia2, views[1]), (ia, views[4])])
        assert counters[:2] == (3, 2), counters
    finally:
        ia2.free()


def test_switch_off_in_a_child_gives_the_same_bytes(ctx, modsx, images, tmp_path):
    assert not os.environ.get("MODSX_VIEWS_SHARE_ROT"), "this module is about the default (sharing on) in the parent"
    a, _ = images[SIZES[1]]
    mine = CH.run_ladder(modsx, ctx, a)
    assert tuple(mine["counters"][:2]) == (30, 18)
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, image=a)
    p = subprocess.run([sys.executable, CHILD, inp, outp], env=dict(os.environ, MODSX_VIEWS_SHARE_ROT="0"), timeout=CHILD_TIMEOUT_S,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode(errors="replace")[-1500:]
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit("the view synthesis child ended with status %d; nothing more is started on the GPU.  Its stderr ended:\n%s"
                    % (p.returncode, err), returncode=1)
    assert p.returncode == 0, "the view synthesis child failed with status %d:\n%s" % (p.returncode, err)
    z = np.load(outp)
    views_fused, groups, rot = (int(x) for x in z["counters"])
    assert (views_fused, groups) == (30, 30), "MODSX_VIEWS_SHARE_ROT=0: groups equal views"
    assert rot > int(mine["counters"][2])
    names = sorted(k for k in mine if k.startswith("view_"))
    assert len(names) == 30 and names == sorted(k for k in z.files if k.startswith("view_"))
    for k in names:
        assert mine[k].tobytes() == z[k].tobytes(), k
