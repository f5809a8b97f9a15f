"""GPU: the description stage against the oracle at every window-size path of its planner (mods_amd/csrc/describe_plan.cpp, driven by
describe_batch in engine.hip) and its five kernels (k_sample_rows_lds fused / row filter only, k_blur_cols_lds, k_patch_sample,
k_patch_blur, k_describe).

For every window size P of tests/describe_cases.py: ONE Context.describe_regions call for its three regions (interior: no-border
sampling; top-left and bottom-right: the border path) against oracle.describe_regions on the same records, np.array_equal.  Which
path the call took is read from the library: the difference of two Context.describe_counters() readings gives the size's signature
(fused or not, row tile clamped to 32 or not, LDS row tiles and LDS column tiles per window, global-memory tiles of each kind).
Every such difference must equal what the planner alone gives for the same regions and options (mods_amd.describe_plan): the
path classes themselves are proven without a device in tests/test_describe_plan_cpu.py, and this equality ties that plan to what
the device call ran.

From the signatures (test_every_path_class_and_both_sides_of_every_change):
  - all seven path classes occur, in this order of P, each a contiguous run: fused; whole-window row tile + one LDS column tile;
    32-row clamp; row tiles of at most 32 rows + one column tile; several column tiles; LDS rows + global-memory column filter;
    all global-memory;
  - where the class changes, the list holds the two sizes 2 apart on either side;
  - the numbers of distinct row-tiles-per-window and column-tiles-per-window values are exactly ROW_TILE_VALUES and
    COL_TILE_VALUES, what the list yields with today's MODSX_SR_WIN, MODSX_FC_ROWS and MODSX_BLUR_LDS_C.  Someone who retunes
    those moves the paths under the list: the test then fails and the list in tests/describe_cases.py has to be derived again.
    (The planner has only 15 column-tile counts to give: above P = 83 every window needs the same 82 columns, and the columns per
    tile, 2..49, give ceil(82 / ro) in {2, 3, 4, 5, 6, 7, 8, 9, 11, 14, 17, 21, 28, 41} -- 10 and 12 are skipped because the tap
    count grows in steps; with the single tile below P = 67 that is 15, and the list reaches every one of them.)

At one size of every class: the descriptor types 0, 2 and 3, photo_norm = 0, fast = 1, calls of 1, 2, 3 and 5 regions (k_describe
takes two regions per workgroup: the odd counts leave its second slot empty) and one call that mixes direct-branch and smoothed
regions.  P = 2331 is refused ("descriptor window too large") before anything is launched.
"""
import numpy as np
import pytest

from tests import describe_cases as DC

pytestmark = pytest.mark.gpu

CLASSES, CLASS_SIZE, PER_WINDOW, ROW_TILE_VALUES, COL_TILE_VALUES = DC.CLASSES, DC.CLASS_SIZE, DC.PER_WINDOW, DC.ROW_TILE_VALUES, DC.COL_TILE_VALUES
_class_of = DC.class_of


def _delta(ctx, before):
    now = ctx.describe_counters()
    return {k: now[k] - before[k] for k in now}


def _same_as_plan(modsx, d, regs, fast=0):
    """what the device call booked (the difference d of two counter readings) is what the planner alone gives for its regions"""
    plan = modsx.describe_plan(regs, DC.MR_SIZE, fast=fast, arena_floats=DC.arena_floats())
    assert plan["rc"] == 0, plan
    assert {k: d[k] for k in DC.SUMMED} == {k: plan["counters"][k] for k in DC.SUMMED}, (d, plan)


@pytest.fixture(scope="module")
def image(ctx):
    im = ctx.upload(DC.image())          # f32 in, f32 on the device
    yield im
    im.free()


@pytest.fixture(scope="module")
def sweep(ctx, image, modsx):
    """every size of the list through the device, once: {P: (descriptors, signature per window)}"""
    out = {}
    for P in DC.SIZES:
        c0 = ctx.describe_counters()
        got = ctx.describe_regions(image, DC.regions_of(P).view(modsx.REGION), mr_size=DC.MR_SIZE)
        d = _delta(ctx, c0)
        assert (d["calls"], d["chunks"], d["jobs"], d["direct_jobs"]) == (1, 1, 3, 0), (P, d)
        _same_as_plan(modsx, d, DC.regions_of(P))
        assert all(d[k] % 3 == 0 for k in PER_WINDOW), "P = %d: three windows of one size, three times the tiles: %r" % (P, d)
        out[P] = (got, {k: d[k] // 3 for k in PER_WINDOW})
    return out


@pytest.mark.parametrize("name,sizes", DC.GROUPS, ids=[g[0] for g in DC.GROUPS])
def test_every_size_equals_oracle(sweep, name, sizes):
    refs = DC.references(sizes)
    bad = []
    for P in sizes:
        got, sig = sweep[P]
        print("P = %4d  %-22s %r" % (P, _class_of(sig), tuple(sig[k] for k in PER_WINDOW)))
        for i, where in enumerate(("interior", "top-left", "bottom-right")):
            if not np.array_equal(got[i], refs[P][i]):
                bad.append("P = %d %s (%s): %d of 128 entries differ, first at %d" % (P, where, _class_of(sig), int((got[i] != refs[P][i]).sum()),
                                                                                    int(np.nonzero(got[i] != refs[P][i])[0][0])))
    assert not bad, "\n".join(bad)


def test_direct_branch_equals_oracle(ctx, image, modsx):
    """s * mr = 7: patchImageSize 15, 15 / 41 <= 0.4, no smoothed window; s * mr = 8 is P = 19 of the sweep"""
    c0 = ctx.describe_counters()
    got = ctx.describe_regions(image, DC.regions_of(0).view(modsx.REGION), mr_size=DC.MR_SIZE)
    d = _delta(ctx, c0)
    assert (d["jobs"], d["direct_jobs"]) == (3, 3) and not any(d[k] for k in PER_WINDOW), d
    assert np.array_equal(got, DC.references((0,))[0])


def test_every_path_class_and_both_sides_of_every_change(sweep):
    cls = [(P, _class_of(sweep[P][1])) for P in DC.SIZES]
    runs = []
    for P, c in cls:
        if not runs or runs[-1][0] != c:
            runs.append([c, P, P])
        runs[-1][2] = P
    print("path classes over P: %r" % (runs,))
    retune = ("the window sizes of tests/describe_cases.py no longer sit where describe_batch changes path (MODSX_SR_WIN, MODSX_FC_ROWS, "
              "MODSX_BLUR_LDS_C or the tile rule were changed?): derive the list again, with both sides of every boundary")
    assert tuple(r[0] for r in runs) == CLASSES, "%s\n%r" % (retune, runs)
    for a, b in zip(runs, runs[1:]):
        assert b[1] - a[2] == 2, "%s\n%s ends at P = %d, %s begins at P = %d" % (retune, a[0], a[2], b[0], b[1])
    for c, P in CLASS_SIZE.items():
        assert dict(cls)[P] == c, "%s\nP = %d is %s, not %s" % (retune, P, dict(cls)[P], c)
    rows = {sweep[P][1]["lds_row_tiles"] for P in DC.SIZES} - {0}
    cols = {sweep[P][1]["lds_col_tiles"] for P in DC.SIZES} - {0}
    print("row tiles per window: %d values %r\ncolumn tiles per window: %d values %r" % (len(rows), sorted(rows), len(cols), sorted(cols)))
    assert len(rows) == ROW_TILE_VALUES and len(rows) >= 25, "%s\n%d row-tile values: %r" % (retune, len(rows), sorted(rows))
    assert len(cols) == COL_TILE_VALUES, "%s\n%d column-tile values: %r" % (retune, len(cols), sorted(cols))
    # k_patch_sample's 64 x 128 tiles: both sides of the 128-column edge, and a ragged edge in both directions
    assert sweep[1023][1]["sample_tiles"] == 16 * 8 and sweep[1025][1]["sample_tiles"] == 17 * 9


@pytest.mark.parametrize("cls", CLASSES)
def test_options_and_region_counts_at_one_size_per_class(ctx, image, modsx, oracle, cls):
    P = CLASS_SIZE[cls]
    five = DC.regions_of(P, (0, 1, 2, 3, 4))
    mixed = np.concatenate([DC.regions_of(0, (3,)), DC.regions_of(P, (1,)), DC.regions_of(0, (0, 4)), DC.regions_of(P, (0, 3)),
                            DC.regions_of(0, (2,))])
    calls = [("desc_type %d" % t, DC.regions_of(P), dict(desc_type=t)) for t in (0, 2, 3)]
    calls.append(("photo_norm 0", DC.regions_of(P), dict(photo_norm=0)))
    calls.append(("fast 1", DC.regions_of(P), dict(fast=1)))
    calls += [("%d regions" % n, five[:n].copy(), {}) for n in (1, 2, 3, 5)]
    calls.append(("direct and smoothed mixed", mixed, {}))
    # the oracle's name for the descriptor type is `rootsift`
    want = DC.oracle_rows([(r, dict(mr_size=DC.MR_SIZE, **{("rootsift" if k == "desc_type" else k): v for k, v in kw.items()})) for _, r, kw in calls])
    bad = []
    for (what, regs, kw), ref in zip(calls, want):
        c0 = ctx.describe_counters()
        got = ctx.describe_regions(image, regs.view(modsx.REGION), mr_size=DC.MR_SIZE, **kw)
        d = _delta(ctx, c0)
        direct = len(regs) if kw.get("fast") else int(sum(DC.window_of(s) == 0 for s in regs["det_kp"]["s"]))
        assert (d["calls"], d["chunks"], d["jobs"], d["direct_jobs"]) == (1, 1, len(regs), direct), (what, d)
        _same_as_plan(modsx, d, regs, fast=kw.get("fast", 0))
        assert ref.any(1).all(), what
        if not np.array_equal(got, ref):
            bad.append("P = %d (%s), %s: rows %r differ" % (P, cls, what, np.nonzero((got != ref).any(1))[0].tolist()))
    # every option is heard by the oracle: the descriptor types and fast = 1 change the descriptor, against the default options
    # too; photo_norm changes the 41 x 41 patch -- RootSIFT's own normalisation absorbs most of a change of gain and offset (at
    # P = 25 all of it, at P = 39 all but 7 entries), so the descriptor alone would not show that the option arrived
    dflt = DC.references((P,))[P]
    assert len({w.tobytes() for w in want[:3] + [want[4], dflt]}) == 5 and len({w.tobytes() for w in want[:5]}) == 5
    patch = oracle.extract_patch(DC.image(), DC.regions_of(P)[:1], mr_size=DC.MR_SIZE)
    assert not np.array_equal(oracle.describe_patch(patch, photo_norm=0)[1], oracle.describe_patch(patch, photo_norm=1)[1])
    assert not bad, "\n".join(bad)


def test_window_with_513_taps_is_refused(ctx, image, modsx):
    c0 = ctx.describe_counters()
    with pytest.raises(RuntimeError, match="descriptor window too large"):
        ctx.describe_regions(image, DC.regions_of(DC.REFUSED_P).view(modsx.REGION), mr_size=DC.MR_SIZE)
    d = _delta(ctx, c0)
    assert d["jobs"] == 0 and not any(d[k] for k in PER_WINDOW), "the refusal comes before any job is planned: %r" % (d,)
    # the context is as usable as before
    assert np.array_equal(ctx.describe_regions(image, DC.regions_of(19).view(modsx.REGION), mr_size=DC.MR_SIZE), DC.references((19,))[19])
