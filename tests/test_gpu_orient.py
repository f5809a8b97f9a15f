"""GPU: k_orientation (mods_amd/csrc/kernels_orient.hip) region by region against the CPU oracle, on the inputs of
tests/orient_cases.py (their claims are proven on the CPU by tests/test_orient_cases_cpu.py).

Planted 41 x 41 patches reach the production kernel through Context.detect_orientation at mr_size 20 (the identity harness): every
bin-table entry, the unread bin 36, 1245 votes in one bin, no votes at all, one lane holding all the votes, exact ties, plateaus,
the Half fold and the cut at maxAngles -- compared bit for bit with oracle.detect_orientation, and the number of angles per region
with the numpy model.  The launch counters say which instance of the kernel ran (bin table in LDS below 8192 regions, in global
memory from 8192 on).  Geometric regions exercise both branches of the sampler, taps outside the image included."""
import numpy as np
import pytest

import orient_cases as cases
import orient_model as M
from common import same_records

pytestmark = pytest.mark.gpu

MAX_ANGS = (-1, 0, 1, 2, cases.MAX_PEAKS - 1, cases.MAX_PEAKS, cases.MAX_PEAKS + 1, 100)
_ref_cache = {}


@pytest.fixture(scope="module")
def planted(ctx, modsx):
    img, centres = cases.compose()
    regs = cases.identity_regions(modsx.REGION, centres)
    im = ctx.upload(img)
    yield dict(img=img, centres=centres, regs=regs, im=im, n=len(regs))
    im.free()


def _oracle_ref(oracle, modsx, planted, half, th, max_ang, upright=0):
    key = (half, th, max_ang, upright)
    if key not in _ref_cache:
        _ref_cache[key] = oracle.detect_orientation(planted["img"], planted["regs"].view(oracle.REGION), mr_size=cases.MR_IDENTITY,
                                                    half=half, max_ang=max_ang, th=th, upright=upright).view(modsx.REGION)
    return _ref_cache[key]


def _groups(recs, counts):
    """records of a list whose region i produced counts[i] of them -> list of per-region slices"""
    ends = np.cumsum(counts)
    assert ends[-1] == len(recs)
    return [recs[e - c:e] for c, e in zip(counts, ends)]


def _oracle_counts(oracle, half, th, max_ang):
    return np.array([len(oracle.dominant_angles(c["patch"], half, th, max_ang)) for c in cases.planted()], np.int64)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("th", [0.8, 1.0])
def test_planted_patches_equal_the_oracle(ctx, modsx, oracle, planted, half, th):
    A = cases.analysis(oracle)
    names = [c["name"] for c in cases.planted()]
    for max_ang in MAX_ANGS:
        before = modsx.orientation_launches()
        got = ctx.detect_orientation(planted["im"], planted["regs"], mr_size=cases.MR_IDENTITY, half=half, max_ang=max_ang, th=th)
        after = modsx.orientation_launches()
        ref = _oracle_ref(oracle, modsx, planted, half, th, max_ang)
        # fewer than 8192 regions: the instance with the bin table in LDS, and only when there is something to orient
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if max_ang > 0 else (0, 0)), max_ang
        model = [len(a) for a in M.dominant_angles_batch(oracle, None, half, th, max_ang, analysis=A)[0]] if max_ang > 0 else [0] * planted["n"]
        per = cases.counts_per_centre(got, planted["centres"])
        wrong = [names[i] for i in np.nonzero(per != np.array(model))[0]]
        assert not wrong, (half, th, max_ang, len(wrong), wrong[:6])
        if not same_records(got, ref):
            gg, rg = _groups(got, per), _groups(ref, cases.counts_per_centre(ref, planted["centres"]))
            bad = [names[i] for i in range(planted["n"]) if not same_records(gg[i], rg[i])]
            assert not bad, (half, th, max_ang, len(bad), bad[:6])
            assert False, "records differ in their order only"
        if max_ang > 0:
            assert len(got) > 0
        else:
            assert len(got) == 0       # DetectOrientation runs the functor only for maxAngNum > 0 (synth-detection.cpp:866)


@pytest.mark.parametrize("half,th,max_ang", [(0, 0.8, 1), (1, 1.0, cases.MAX_PEAKS), (0, 0.8, 0), (1, 0.8, -1), (0, 1.0, 100)])
def test_planted_patches_with_upright_copies(ctx, modsx, oracle, planted, half, th, max_ang):
    got = ctx.detect_orientation(planted["im"], planted["regs"], mr_size=cases.MR_IDENTITY, half=half, max_ang=max_ang, th=th, upright=1)
    ref = _oracle_ref(oracle, modsx, planted, half, th, max_ang, upright=1)
    assert len(ref) >= planted["n"] and same_records(got, ref)
    without = ctx.detect_orientation(planted["im"], planted["regs"], mr_size=cases.MR_IDENTITY, half=half, max_ang=max_ang, th=th)
    assert len(got) == len(without) + planted["n"]


@pytest.mark.parametrize("n,instance", [(8191, "lds"), (8192, "global"), (8193, "global")])
def test_both_table_paths_at_the_boundary(ctx, modsx, oracle, planted, n, instance):
    """the list tiled to n regions: every copy of a region gives the bytes of the oracle's single evaluation, whichever instance ran"""
    half, th, max_ang = 0, 0.8, 2
    assert modsx.orientation_tables()["global_table_from"] == 8192
    ref = _oracle_ref(oracle, modsx, planted, half, th, max_ang)
    groups = _groups(ref, _oracle_counts(oracle, half, th, max_ang))
    order = np.arange(n) % planted["n"]
    regs = planted["regs"][order]
    want = np.concatenate([groups[i] for i in order])
    modsx.orientation_launches(reset=True)
    got = ctx.detect_orientation(planted["im"], regs, mr_size=cases.MR_IDENTITY, half=half, max_ang=max_ang, th=th)
    assert modsx.orientation_launches() == ((1, 0) if instance == "lds" else (0, 1))
    assert len(got) == len(want) and same_records(got, want)
    if instance == "global":
        # and with the fold, every peak and the unread bin: the other instance on the cases that plant table entries
        ref = _oracle_ref(oracle, modsx, planted, 1, 1.0, 18)
        groups = _groups(ref, _oracle_counts(oracle, 1, 1.0, 18))
        got = ctx.detect_orientation(planted["im"], regs, mr_size=cases.MR_IDENTITY, half=1, max_ang=18, th=1.0)
        assert modsx.orientation_launches() == (0, 2)
        assert same_records(got, np.concatenate([groups[i] for i in order]))


def _mixed_order(n_all):
    """a list that starts with the edge cases (extremes, peaks, named ramps) and goes on through every family"""
    names = [c["name"] for c in cases.planted()]
    first = [i for i, s in enumerate(names) if s.startswith(("extreme/", "peaks/"))]
    rest = [i for i in range(0, n_all, 29) if i not in first]
    return np.array(first[::2] + rest + first[1::2])


@pytest.mark.parametrize("half,max_ang", [(0, 2), (1, 18)])
def test_launch_geometry_prefixes(ctx, modsx, oracle, planted, half, max_ang):
    """n = 1 .. 17 (grids with empty blocks: xcd_chunk with n no multiple of 8) and an odd count near 100: every region gives the
    records it gives in the full run"""
    th = 0.8
    ref = _oracle_ref(oracle, modsx, planted, half, th, max_ang)
    groups = _groups(ref, _oracle_counts(oracle, half, th, max_ang))
    order = _mixed_order(planted["n"])
    assert len(order) >= 101
    full = ctx.detect_orientation(planted["im"], planted["regs"], mr_size=cases.MR_IDENTITY, half=half, max_ang=max_ang, th=th)
    assert same_records(full, ref)
    for n in list(range(1, 18)) + [101]:
        sel = order[:n]
        got = ctx.detect_orientation(planted["im"], planted["regs"][sel], mr_size=cases.MR_IDENTITY, half=half, max_ang=max_ang, th=th)
        want = np.concatenate([groups[i] for i in sel])
        assert len(got) == len(want) and same_records(got, want), n


@pytest.mark.parametrize("which", ["textured", "small"])
def test_geometric_cases_equal_the_oracle(ctx, modsx, oracle, which):
    img = cases.textured_image() if which == "textured" else cases.small_image()
    group = cases.GEOMETRIC if which == "textured" else cases.SMALL_GEOMETRIC
    regs = cases.geometric_regions(modsx.REGION, group)
    im = ctx.upload(img)
    rows, cols = img.shape
    try:
        for mr in cases.MR_SIZES:
            passing = int((~modsx.check_borders([cases.border_tuples(c[1], mr, rows, cols)[0] for c in group])).sum())
            assert 0 < passing < len(group)
            for half in (0, 1):
                for max_ang in (1, 5):
                    ref = oracle.detect_orientation(img, regs.view(oracle.REGION), mr_size=mr, half=half, max_ang=max_ang).view(modsx.REGION)
                    # (the pair / view pipelines count here too; detect_orientation launches every region that passes the box)
                    before = modsx.orientation_counts()
                    got = ctx.detect_orientation(im, regs, mr_size=mr, half=half, max_ang=max_ang)
                    after = modsx.orientation_counts()
                    assert after[0] - before[0] == passing and after[1] == before[1], (mr, half, max_ang)
                    assert same_records(got, ref), (which, mr, half, max_ang)
                    up = ctx.detect_orientation(im, regs, mr_size=mr, half=half, max_ang=max_ang, upright=1)
                    assert len(up) == len(got) + passing
                    assert same_records(up, oracle.detect_orientation(img, regs.view(oracle.REGION), mr_size=mr, half=half,
                                                                      max_ang=max_ang, upright=1).view(modsx.REGION))
                    # each region alone (n = 1) gives what it gives in the batch
                    alone = [ctx.detect_orientation(im, regs[i:i + 1], mr_size=mr, half=half, max_ang=max_ang) for i in range(len(regs))]
                    assert same_records(np.concatenate(alone), got), (which, mr, half, max_ang)
                    for (name, _, claims), a in zip(group, alone):
                        if claims.get(mr) == "dropped":
                            assert len(a) == 0, name
    finally:
        im.free()


def test_idempotence_same_and_fresh_context(ctx, modsx, oracle, planted):
    """the patch buffer in LDS is reused for counters and sorted weights within a launch: the same call twice, and on a fresh
    context, gives the same bytes"""
    args = dict(mr_size=cases.MR_IDENTITY, half=1, max_ang=3, th=0.8)
    first = ctx.detect_orientation(planted["im"], planted["regs"], **args)
    again = ctx.detect_orientation(planted["im"], planted["regs"], **args)
    assert same_records(first, again) and same_records(first, _oracle_ref(oracle, modsx, planted, 1, 0.8, 3))
    fresh = modsx.Context(0)
    try:
        im = fresh.upload(planted["img"])
        other = fresh.detect_orientation(im, planted["regs"], **args)
        reversed_list = fresh.detect_orientation(im, planted["regs"][::-1].copy(), **args)
        im.free()
    finally:
        fresh.close()
    assert same_records(first, other)
    per = cases.counts_per_centre(first, planted["centres"])
    want = np.concatenate(_groups(first, per)[::-1])
    assert same_records(reversed_list, want)
