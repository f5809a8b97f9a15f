"""The images and parameter sets of the SURF detector tests (tests/test_surfdet_model_cpu.py, tests/test_gpu_surfdet.py,
tools/make_surfdet_fixture.py): seeded f32 images with values 0 .. 255, built once per process and left alone.  Sizes are
width x height.  What a case claims to reach is checked against the model's report in tests/test_surfdet_model_cpu.py.

Images:
  blobs(w, h)     gaussian blobs of sigma 1.5 .. 50 px of both polarities on a textured ground: every octave has maxima;
  dots(w, h)      a jittered 7 px grid of dots of sigma 1.6 .. 3 of both polarities: thousands of extrema at thresh = 0 and
                  init_sample = 1;
  flat(w, h)      one value everywhere: every response is 0, no point;
  borders(w, h)   blobs centred on all four borders and corners, where BoxIntegral's clamps act.
Cases (name -> image, parameters):
  every size at the parameters the issue names for it (the ini's unless stated), then the parameter sets on the 320 x 240 image:
  init_sample 1, 3, 6, octaves 1 and 0 (0 gives five), thresh 0 (thousands of points) and -1 (gives the default), and a 400 x 400
  image at init_sample 1 with five octaves, the smallest round size whose fifth octave has room for a point (its t layers are
  25 x 25 with a border of 9)."""
import functools

import numpy as np

import surfdet_model as M

INI = dict(M.INI)


def _ground(w, h, rng):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = 118.0 + 9.0 * np.sin(x * 0.71 + y * 0.37) + 7.0 * np.sin(x * 0.23 - y * 0.53) + rng.uniform(-6.0, 6.0, (h, w))
    return g, x, y


def _finish(g):
    out = np.clip(g, 0.0, 255.0).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def blobs(w, h, seed=0, centre=0.0):
    rng = np.random.default_rng(7000 + seed + 131 * w + h)
    g, x, y = _ground(w, h, rng)
    if centre:          # one blob of this sigma on the fifth octave's grid (multiples of 16) near the centre: its few candidates lie there
        g += 100.0 * np.exp(-((x - w // 32 * 16) ** 2 + (y - h // 32 * 16) ** 2) / (2.0 * centre * centre))
    lim = min(w, h) / 5.0
    sigmas = [s for s in (1.5, 2.0, 2.5, 3.2, 4.0, 5.0, 6.5, 8.0, 10.0, 13.0, 16.0, 20.0, 25.0, 32.0, 40.0, 50.0) if s <= max(lim, 2.0)]
    if centre:          # ... and no other blob of the two coarsest octaves' sizes competes with it
        sigmas = [s for s in sigmas if s <= 16.0]
    for k in range(max(6, w * h // 1500)):
        s = sigmas[k % len(sigmas)]
        m = min(3.0 * s, w / 2.0 - 1, h / 2.0 - 1)
        cx, cy = rng.uniform(m, w - m), rng.uniform(m, h - m)
        amp = (1.0 if k % 2 else -1.0) * rng.uniform(60.0, 110.0)
        g += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))
    return _finish(g)


@functools.lru_cache(maxsize=None)
def dots(w, h):
    rng = np.random.default_rng(7700 + w + h)
    g, x, y = _ground(w, h, rng)
    k = 0
    for gy in range(4, h - 3, 7):
        for gx in range(4, w - 3, 7):
            cx, cy, s = gx + rng.uniform(-1.5, 1.5), gy + rng.uniform(-1.5, 1.5), rng.uniform(1.6, 3.0)
            y0, y1, x0, x1 = max(0, gy - 12), min(h, gy + 13), max(0, gx - 12), min(w, gx + 13)
            amp = (1.0 if k % 2 else -1.0) * rng.uniform(50.0, 110.0)
            g[y0:y1, x0:x1] += amp * np.exp(-((x[y0:y1, x0:x1] - cx) ** 2 + (y[y0:y1, x0:x1] - cy) ** 2) / (2.0 * s * s))
            k += 1
    return _finish(g)


@functools.lru_cache(maxsize=None)
def flat(w, h):
    return _finish(np.full((h, w), 128.0))


@functools.lru_cache(maxsize=None)
def borders(w, h):
    rng = np.random.default_rng(7900 + w + h)
    g, x, y = _ground(w, h, rng)
    spots = [(0, h / 2), (w - 1, h / 2), (w / 2, 0), (w / 2, h - 1), (0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1),
             (w / 3, h / 3), (2 * w / 3, 2 * h / 3), (w / 4, 3 * h / 4)]
    for k, (cx, cy) in enumerate(spots):
        s = (3.0, 5.0, 8.0, 12.0)[k % 4]
        g += (100.0 if k % 2 else -100.0) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))
    return _finish(g)


def _p(**kw):
    p = dict(INI)
    p.update(kw)
    return p


@functools.lru_cache(maxsize=None)
def _build():
    c = []
    add = lambda name, img, **kw: c.append((name, img, _p(**kw)))                 # noqa: E731
    add("s30x30_is1", blobs(30, 30), init_sample=1)
    add("s31x33_is1", blobs(31, 33), init_sample=1)
    for w in (63, 64, 65, 129):
        add("s%dx48" % w, blobs(w, 48))
    add("s239x300_is1_o5", blobs(239, 300), init_sample=1, octaves=0)
    add("s478x480_is2_o5", blobs(478, 480), init_sample=2, octaves=0)
    add("s320x240", blobs(320, 240))
    add("flat_320x240", flat(320, 240))
    add("flat_65x48_t0", flat(65, 48), thresh=0.0)
    add("borders_320x240", borders(320, 240))
    add("borders_129x48_is1", borders(129, 48), init_sample=1)
    for s in (1, 3, 6):
        add("s320x240_is%d" % s, blobs(320, 240), init_sample=s)
    add("s320x240_o1", blobs(320, 240), octaves=1)
    add("s320x240_o0", blobs(320, 240), octaves=0)
    add("dots320x240_is1_t0", dots(320, 240), init_sample=1, thresh=0.0)
    add("s400x400_is1_o5", blobs(400, 400, centre=40.0), init_sample=1, octaves=0)
    add("s320x240_tneg", blobs(320, 240), thresh=-1.0)
    add("s320x240_iv9", blobs(320, 240), intervals=9)
    return tuple(c)


BATCH = ("s65x48", "s320x240", "borders_129x48_is1")     # the mixed batch: three sizes; detect at the ini's parameters
WHOLE_PLANES = ("s30x30_is1", "s31x33_is1")              # the fixture keeps every plane of these two


def cases():
    return list(_build())


def names():
    return [n for n, _, _ in _build()]


def case(name):
    return next(c for c in _build() if c[0] == name)


_MODEL = {}


def model(name):
    """surfdet_model.detect of the case, computed once per process"""
    if name not in _MODEL:
        _, img, par = case(name)
        _MODEL[name] = M.detect(img, **par)
    return _MODEL[name]


def model_of(img, **par):
    key = (id(img), tuple(sorted(par.items())))
    if key not in _MODEL:
        _MODEL[key] = M.detect(img, **par)
    return _MODEL[key]
