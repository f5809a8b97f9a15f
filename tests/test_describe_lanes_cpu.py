"""Which lane does which element in the LDS describe kernels (mods_amd/csrc/describe_lanes.hpp), checked on the CPU through the
host-only entries mods_amd.describe_lane_map and mods_amd.describe_lanes -- the same header the kernels compile.

* the tap slots of a parked chunk: for every row count of a row pass (1 .. 64) and every chunk width the rule can produce, the
  enumeration e -> (row, column) is a bijection onto rows x nc, its multiply-shift quotient is e // nc, and the coordinate words it
  reads stay inside the wavefront's park at an odd row stride;
* slot utilisation over the window sizes of one image of the benchmark scene (synthetic.blob_image(768, 1024, 5500, 12345) under the
  31 views, described by the oracle): the share of issued lane slots that hold a sample or an output pair, filters weighted by
  their tap count.  The floors sit below what issuing the remainder in whole wavefronts can reach (0.93 / 0.96 / 0.94 / 0.98),
  with room for the granularity of a chunk; the rule before this one, restated in the library for comparison, must give the
  0.48 / 0.60 / 0.41 / 0.77 it was measured at, which keeps the model honest.
"""
import functools

import numpy as np
import pytest

import mods_amd
from mods_amd import synthetic

from describe_cases import window_of

DESC_MR = 5.1962
FLOORS = dict(sample=0.80, rows=0.90, cols_fused=0.90, cols=0.95)
PARENT = dict(sample=0.48, rows=0.60, cols_fused=0.41, cols=0.77)


@pytest.mark.parametrize("rows", range(1, 65))
def test_chunk_enumeration_is_a_bijection(rows):
    rule = mods_amd.describe_lane_map(rows)
    full, stride, park = rule["cols"], rule["stride"], rule["park_words"]
    assert 1 <= full <= 63 and stride % 2 == 1 and stride >= full
    assert rows * stride <= park                                  # lane-per-row writes of a full chunk stay inside the park
    assert rows * full <= 256 < rows * (full + 1) or full == 63   # as many columns as four slots hold
    for nc in range(1, full + 1):
        got = mods_amd.describe_lane_map(rows, nc)
        m, tot = got["map"], rows * nc
        assert len(m) == tot and got["slots"] == -(-tot // 64) and got["slots"] <= 4
        e = np.arange(tot)
        assert np.array_equal(m[:, 0], e // nc), (rows, nc)       # the multiply-shift quotient, every e of the range
        assert np.array_equal(m[:, 1], e % nc), (rows, nc)
        assert len({(int(r), int(c)) for r, c, _ in m}) == tot    # onto rows x nc, no sample twice
        assert np.array_equal(m[:, 2], m[:, 0] * stride + m[:, 1])
        assert m[:, 2].min() >= 0 and m[:, 2].max() < park
        assert (e * got["magic"]).max() < 1 << 24                 # the product is a 24-bit multiply


def test_chunk_rule_refuses_what_it_cannot_produce():
    for rows, nc in ((0, 1), (65, 1), (64, 5), (12, 22), (3, -1)):
        with pytest.raises(Exception):
            mods_amd.describe_lane_map(rows, nc)


@functools.lru_cache(maxsize=None)
def _scene_windows():
    """window sizes of the regions of one benchmark image (about 2 s of oracle time), as {P: count}"""
    from oracle import pyoracle as O
    img = synthetic.blob_image(768, 1024, 5500, 12345)
    views = O.set_vs_pars([1.0], [1.0, 2.0, 4.0, 6.0, 8.0], 120.0, 0.2, 1, [])
    assert len(views) == 31
    regs, _ = O.detect_describe_views(img, views, threads=8)
    P = np.array([window_of(float(s), DESC_MR) for s in regs["det_kp"]["s"]])
    P = P[P > 0]
    sizes, counts = np.unique(P, return_counts=True)
    return dict(zip((int(p) for p in sizes), (int(c) for c in counts)))


@functools.lru_cache(maxsize=None)
def _utilisation():
    """{phase: (this build, the rule before it)}: useful / issued lane slots over the scene's windows, filters weighted by taps"""
    tot = {ph: np.zeros(3) for ph in mods_amd.DESCRIBE_LANE_PHASES}
    for P, cnt in _scene_windows().items():
        k = mods_amd.describe_lanes(P)
        for ph in mods_amd.DESCRIBE_LANE_PHASES:
            w = cnt * (1 if ph == "sample" else k["ksize"])
            tot[ph] += w * np.array(k[ph], np.float64)
    return {ph: (t[0] / t[1], t[0] / t[2]) for ph, t in tot.items()}


def test_scene_is_the_one_the_model_was_made_on():
    w = _scene_windows()
    P = np.repeat(list(w.keys()), list(w.values()))
    assert len(P) == 25593 and P.max() == 349
    assert [int(v) for v in np.percentile(P, [1, 10, 25, 50, 75, 90, 99], method="nearest")] == [23, 25, 31, 41, 59, 81, 151]


@pytest.mark.parametrize("phase", mods_amd.DESCRIBE_LANE_PHASES)
def test_slot_utilisation_of_this_build(phase):
    now, _ = _utilisation()[phase]
    print("%s: %.4f of the issued slots hold work (floor %.2f)" % (phase, now, FLOORS[phase]))
    assert now >= FLOORS[phase]
    assert now <= 1.0


@pytest.mark.parametrize("phase", mods_amd.DESCRIBE_LANE_PHASES)
def test_parent_rule_restated(phase):
    _, before = _utilisation()[phase]
    print("%s: the rule before gave %.4f (measured %.2f)" % (phase, before, PARENT[phase]))
    assert abs(before - PARENT[phase]) <= 0.01
