"""The images, parameter sets and planted Ldet planes of the KAZE detector tests (tests/test_kaze_model_cpu.py,
tests/test_gpu_kaze.py, tools/make_kaze_fixture.py): seeded f32 images with values 0 .. 255 from tests/surfdet_cases.py, built
once per process and left alone.  Sizes are width x height.  What a case claims to reach is checked against the model's report in
tests/test_kaze_model_cpu.py.

Image cases (name -> image, parameters; the defaults of AKAZEOptions unless stated):
  t48x40, t61x50     the two smallest: one octave, no room for a keypoint; the fixture keeps every plane of these two;
  s128x96 .. s640x320  1, 2, 3 and 4 surviving octaves;
  s177x145, s176x145 the general area resize, on both axes and on the rows alone;
  s159x96 / s160x96, s176x79 / s176x80   the 80 x 40 cut on each side: one octave / two octaves;
  s160x96 also has an octave (80 x 48) with maxima none of which lies inside the smax margin;
  flat_128x96        one value everywhere: k = 0, NaN planes, no keypoint;
  s176x144_p12       kcontrast_percentile 1.2: the histogram walk ends below its threshold, k = 0.03;
  s176x144_msurf     descriptor 3 (M-SURF): smax = 12 sqrt(2);
  borders_176x144    blobs on all four borders and corners.
Planted cases (name -> image size, parameters, peaks): Ldet planes of zeros with 3 x 3 peaks, see planted()."""
import functools

import numpy as np

import kaze_model as M
from surfdet_cases import blobs, borders, flat


@functools.lru_cache(maxsize=None)
def _build():
    c = []
    add = lambda name, img, **kw: c.append((name, img, M.params(**kw)))           # noqa: E731
    add("t48x40", blobs(48, 40))
    add("t61x50", blobs(61, 50))
    add("s128x96", blobs(128, 96))
    add("s176x144", blobs(176, 144))
    add("s352x288", blobs(352, 288))
    add("s640x320", blobs(640, 320))
    add("s177x145", blobs(177, 145))
    add("s176x145", blobs(176, 145))
    add("s159x96", blobs(159, 96))
    add("s160x96", blobs(160, 96))
    add("s176x79", blobs(176, 79))
    add("s176x80", blobs(176, 80))
    add("flat_128x96", flat(128, 96))
    add("s176x144_p12", blobs(176, 144), kcontrast_percentile=1.2)
    add("s176x144_msurf", blobs(176, 144), descriptor=3)
    add("borders_176x144", borders(176, 144))
    return tuple(c)


WHOLE_PLANES = ("t48x40", "t61x50")                      # the fixture keeps every plane of these two
BATCH = ("s128x96", "s177x145", "t61x50", "s176x80")     # the mixed batch: four sizes, 1 and 2 octaves, both resize paths
OCTAVES = {"s128x96": 1, "s176x144": 2, "s352x288": 3, "s640x320": 4, "s159x96": 1, "s160x96": 2, "s176x79": 1, "s176x80": 2}

# a 3 x 3 peak relative to its centre value: rows top to bottom.  PLAIN refines to the offsets (0.1, 0.05); FAR to an offset beyond
# 1 (Dx = 0.1, Dxx = Dyy = -1, Dxy = 0.95: x0 = 0.1 / 0.0975); SINGULAR has Dxx = Dyy = -1 and Dxy = 1 exactly: determinant 0
PLAIN = ((0.2, 0.45, 0.2), (0.4, 1.0, 0.6), (0.2, 0.55, 0.2))
FAR = ((0.9, 0.5, -1.0), (0.4, 1.0, 0.6), (-1.0, 0.5, 0.9))
SINGULAR = ((0.75, 0.5, -1.25), (0.5, 1.0, 0.5), (-1.25, 0.5, 0.75))

# (level, row, col, value, pattern)
_SCAN_A = (
    (3, 100, 100, 0.5, PLAIN), (3, 100, 104, 0.75, PLAIN),      # same level, the later one stronger: replaces the entry
    (3, 100, 150, 0.75, PLAIN), (3, 100, 154, 0.5, PLAIN),      # same level, the later one weaker: dropped
    (0, 60, 60, 0.5, PLAIN), (1, 60, 60, 0.875, PLAIN),         # lower level, the upper one stronger: replaces the entry
    (0, 60, 120, 0.875, PLAIN), (1, 60, 121, 0.5, PLAIN),       # lower level, the upper one weaker: dropped
    (0, 5, 100, 0.5, PLAIN), (0, 282, 100, 0.5, PLAIN), (0, 100, 5, 0.5, PLAIN), (0, 100, 346, 0.5, PLAIN),   # out on each side
    (3, 100, 200, 0.625, PLAIN), (4, 50, 100, 0.75, PLAIN),     # the lower level is of the octave below: replaces the entry
    (4, 50, 60, 0.625, PLAIN),                                  # a plain point of octave 1
    (0, 200, 60, 1.0, FAR), (0, 200, 90, 0.5, PLAIN), (0, 200, 120, 1.0, SINGULAR),    # erased; solved; singular after a solved point
)
_SCAN_B = (
    (0, 60, 60, 1.0, SINGULAR),                                 # singular as the first point: the offsets are still zero
    (0, 70, 100, 0.5, PLAIN), (1, 70, 101, 0.875, PLAIN),       # the nearest thing to an upper-level rejection (see the CPU test)
    (0, 100, 40, 0.5, PLAIN), (2, 100, 80, 0.5, PLAIN),
)
PLANTED = {"scan_a": ((352, 288), M.params(), _SCAN_A), "scan_b": ((176, 144), M.params(descriptor=3), _SCAN_B)}


def cases():
    return list(_build())


def names():
    return [n for n, _, _ in _build()]


def case(name):
    return next(c for c in _build() if c[0] == name)


@functools.lru_cache(maxsize=None)
def planted(name):
    """-> (levels, parameters, Ldet planes) of a planted case"""
    (w, h), par, peaks = PLANTED[name]
    lv, _ = M.levels(h, w, **par)
    planes = [np.zeros((L["rows"], L["cols"]), np.float32) for L in lv]
    for level, r, c, v, pat in peaks:
        planes[level][r - 1:r + 2, c - 1:c + 2] = np.float32(v) * np.array(pat, np.float32)
    for p in planes:
        p.setflags(write=False)
    return lv, par, planes


_MODEL = {}


def model(name):
    """kaze_model.detect of the case (kaze_model.scan of a planted case), computed once per process"""
    if name not in _MODEL:
        if name in PLANTED:
            lv, par, planes = planted(name)
            _MODEL[name] = M.scan(planes, lv, **par)
        else:
            _, img, par = case(name)
            _MODEL[name] = M.detect(img, **par)
    return _MODEL[name]
