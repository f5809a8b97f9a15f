"""CPU: which views of a launch set share one rotation in the fused view kernel (mods_amd/csrc/views_plan.cpp: group_views), through
mods_amd.view_plan / mods_amd.views_groups (modsx_debug_view_plan, modsx_debug_views_groups: no device, no context).

Views of one source image whose inverse rotation matches bit for bit are rotated once per tile.  The figures of the default ladder
(30 views, 18 angles, 23 499 562 rotated pixels against 38 613 026) come from GenerateSynthImageCorr's size formulas, evaluated
independently below.  tests/test_gpu_views_shared_rotation.py asserts that a device call books what this rule says.
"""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

ROWS, COLS = 768, 1024
LADDERS = {   # name -> (tilt set, Phi, views, distinct angles as exact fractions of pi, groups)
    "views31": ([1, 2, 4, 6, 8], 120.0, 31, 18, 18),
    # 36 distinct angles; at 5 pi / 6 tilt 6's (pi / 18) * 15 is the double next to (pi / 6) * 5 = (pi / 12) * 10 = (pi / 24) * 20, so
    # that angle is two groups
    "views61": ([1, 2, 4, 6, 8], 60.0, 61, 36, 37),
    "views11": ([1, 2, 4, 6, 8], 360.0, 11, 6, 6),
    "views8": ([1, 2, 3, 4, 6], 360.0, 8, 4, 4),
}


def _plans(modsx, tilts, phi, rows=ROWS, cols=COLS, sigma=0.2, scales=(1.0,)):
    views = modsx.set_vs_pars(list(scales), tilts, phi, sigma, 1, [])
    plans = [modsx.view_plan(rows, cols, v) for v in views]
    keep = [i for i, p in enumerate(plans) if not p["identity"]]
    return [views[i] for i in keep], [plans[i] for i in keep], len(views)


def _rot_size(phi, w, h):
    """w_rot, h_rot of GenerateSynthImageCorr (synth-detection.cpp), restated"""
    if 0 <= phi < math.pi / 2:
        return math.floor(0.5 + math.cos(phi) * w + math.sin(phi) * h), math.floor(0.5 + math.sin(phi) * w + math.cos(phi) * h)
    return math.floor(0.5 - math.cos(phi) * w + math.sin(phi) * h), math.floor(0.5 + math.sin(phi) * w - math.cos(phi) * h)


def _bits(x):
    return struct.pack("<d", x)


def test_default_ladder_rotates_18_angles_instead_of_30_views(modsx):
    views, plans, nv = _plans(modsx, *LADDERS["views31"][:2])
    assert nv == 31 and len(plans) == 30 and all(p["kind"] == 2 for p in plans)
    g = modsx.views_groups(plans)
    assert (g["views_fused"], g["groups"]) == (30, 18)
    assert (g["rotated_pixels"], g["rotated_pixels_alone"]) == (23499562, 38613026)
    # the same figures from the size formulas alone: one rotated image per distinct angle / per view
    area = {}
    for v in views:
        w, h = _rot_size(v.phi, COLS, ROWS)
        area[_bits(v.phi)] = w * h
    assert sum(area.values()) == 23499562 and sum(area[_bits(v.phi)] for v in views) == 38613026
    # which tilts share an angle: 0, 60, 120 degrees are in every tilt's set, 30, 90, 150 in those of 4 and 8
    by_group = {}
    for v, k in zip(views, g["group"]):
        by_group.setdefault(int(k), []).append((round(math.degrees(v.phi)), v.tilt))
    sets = sorted((a[0][0], tuple(t for _, t in a)) for a in by_group.values())
    assert [s for s in sets if len(s[1]) == 4] == [(d, (2.0, 4.0, 6.0, 8.0)) for d in (0, 60, 120)], sets
    assert [s for s in sets if len(s[1]) == 2] == [(d, (4.0, 8.0)) for d in (30, 90, 150)], sets
    assert sorted(t for s in sets if len(s[1]) == 1 for t in s[1]) == [6.0] * 6 + [8.0] * 6, sets
    # one tile grid per group
    tiles = sum(-(-w // 128) * -(-h // 16) for w, h in (_rot_size(struct.unpack("<d", b)[0], COLS, ROWS) for b in area))
    assert g["tiles"] == tiles


def test_members_lie_together_in_the_job_table_and_groups_open_in_view_order(modsx):
    _, plans, _ = _plans(modsx, *LADDERS["views31"][:2])
    g = modsx.views_groups(plans)
    order, group = list(g["order"]), list(g["group"])
    assert sorted(order) == list(range(len(plans)))
    table = [group[i] for i in order]
    assert table == sorted(table), "a group's members are adjacent and groups are numbered in table order: %r" % (table,)
    for k in set(group):
        members = [i for i in order if group[i] == k]
        assert members == sorted(members), "members keep the view order inside a group"
    firsts = [min(i for i in range(len(group)) if group[i] == k) for k in range(g["groups"])]
    assert firsts == sorted(firsts), "a group opens where the view order has its first member"


@pytest.mark.parametrize("name", ["views61", "views11", "views8"])
def test_shipped_view_sets_group_by_angle(modsx, name):
    tilts, phi, nviews, nangles, ngroups = LADDERS[name]
    views, plans, nv = _plans(modsx, tilts, phi)
    assert nv == nviews and len(plans) == nviews - 1
    # the angles the tilt sets prescribe, exactly: r / floor(180 t / Phi) of pi
    exact = {Fraction(r, math.floor(180.0 * t / phi)) for t in tilts if t != 1 for r in range(math.floor(180.0 * t / phi))}
    assert len(exact) == nangles
    doubles = {_bits(v.phi) for v in views}
    g = modsx.views_groups(plans)
    print("%s: %d views, %d angles, %d distinct phi doubles, %d groups, %d of %d rotated pixels" % (
        name, len(plans), nangles, len(doubles), g["groups"], g["rotated_pixels"], g["rotated_pixels_alone"]))
    assert g["views_fused"] == nviews - 1
    assert g["groups"] == len(doubles) == ngroups
    assert g["rotated_pixels"] == sum(w * h for w, h in (_rot_size(struct.unpack("<d", b)[0], COLS, ROWS) for b in doubles))


def test_two_source_images_never_share_a_group(modsx):
    _, plans, _ = _plans(modsx, *LADDERS["views31"][:2])
    one = modsx.views_groups(plans)
    two = modsx.views_groups(plans + plans, sources=[0] * 30 + [1] * 30)
    assert two["groups"] == 2 * one["groups"] and two["rotated_pixels"] == 2 * one["rotated_pixels"]
    grp = list(two["group"])
    assert not set(grp[:30]) & set(grp[30:])
    # ... nor two images of different sizes whose rotations are the same matrices (phi = 0: R is the identity whatever the size)
    v = modsx.make_view(2.0, 0.0, 1.0, 0.2, 1)
    a, b = modsx.view_plan(100, 200, v), modsx.view_plan(100, 201, v)
    assert np.array_equal(a["rinv"], b["rinv"])
    assert modsx.views_groups([a, b])["groups"] == 2 and modsx.views_groups([a, a])["groups"] == 1


def test_cap_splits_a_long_group(modsx):
    plans = [modsx.view_plan(ROWS, COLS, modsx.make_view(t, math.pi / 3, 1.0, 0.2, 1)) for t in (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)]
    g = modsx.views_groups(plans)
    assert modsx.VIEW_GROUP_CAP == 8
    assert list(g["group"]) == [0] * 8 + [1] * 3 and g["groups"] == 2
    assert g["rotated_pixels"] * 11 == g["rotated_pixels_alone"] * 2
    g = modsx.views_groups(plans, cap=3)
    assert list(g["group"]) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3]
    g = modsx.views_groups(plans, cap=1)
    assert list(g["group"]) == list(range(11)) and g["rotated_pixels"] == g["rotated_pixels_alone"]


def test_one_bit_of_rinv_keeps_views_apart(modsx):
    base = modsx.view_plan(ROWS, COLS, modsx.make_view(4.0, math.pi / 3, 1.0, 0.2, 1))
    other = modsx.view_plan(ROWS, COLS, modsx.make_view(8.0, math.pi / 3, 1.0, 0.2, 1))
    assert base["rinv"].tobytes() == other["rinv"].tobytes()
    assert modsx.views_groups([base, other])["groups"] == 1
    for q in range(6):
        off = dict(other)
        r = other["rinv"].copy()
        r[q:q + 1].view(np.uint64)[0] ^= 1       # the last bit of one of the six doubles
        off["rinv"] = r
        assert abs(r[q] - other["rinv"][q]) <= abs(r[q]) * 2.3e-16
        g = modsx.views_groups([base, off])
        assert g["groups"] == 2 and list(g["group"]) == [0, 1], q
    # a size of the rotated image that differs keeps them apart as well
    off = dict(other)
    off["w_rot"] += 1
    assert modsx.views_groups([base, off])["groups"] == 2


def test_views_off_the_fused_launch_stay_out_of_every_group(modsx):
    """A blur beyond the tile's halo (zoom 0.125 at InitSigma 0.5: 7 rows of taps) and a view without a blur keep the separate
    launches; their partners of the same angle are grouped without them."""
    phi = math.pi / 3
    views = [modsx.make_view(2.0, phi, 1.0, 0.5, 1), modsx.make_view(2.0, phi, 0.125, 0.5, 1), modsx.make_view(4.0, phi, 1.0, 0.5, 1),
             modsx.make_view(4.0, phi, 1.0, 0.5, 0)]
    plans = [modsx.view_plan(150, 203, v) for v in views]
    assert [p["kind"] for p in plans] == [2, 0, 2, 0] and plans[1]["ky"] == 7
    g = modsx.views_groups(plans)
    assert list(g["group"]) == [0, -1, 0, -1] and list(g["order"]) == [0, 2, 1, 3]
    assert (g["views_fused"], g["groups"]) == (2, 1)
