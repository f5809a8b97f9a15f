"""The patches and mrSize values of the SURF tests (tests/test_surf_model_cpu.py, tests/test_gpu_surf.py,
tools/make_surf_fixture.py): 41 x 41 f32, from integer formulas, seeded numpy or the oracle's patch extraction, built once per
process and left alone.  cases() -> list of (name, patch).  What a name claims is checked against the model in
tests/test_surf_model_cpu.py, never assumed.

Families:
  random_*          seeded uniform values in [0, 255], full mantissas;
  levels_*          seeded integer grey levels 0 .. 255;
  region_*          the oracle's photonormalised patches of regions on describe_cases.image(): what DescribeRegions<> hands over;
  constant, zero, saturated   one value everywhere (128.5, 0, 255): every response is 0 or, where the window leaves the patch on
                    the far side, the rounding residue of (A - B) - A + B; zero gives len = 0 and a row of NaN;
  step_x, step_y    two-valued halves;
  pixel_*           one pixel of 255 on zeros, at each corner and at the centre;
  bright_flat_*     250 + a fraction, full mantissas: box sums of windows beyond the far border cancel to small values of either
                    sign, the negative ones are clamped;
  bright_holes_*    the same with 3 x 3 holes of zeros: a Haar box that lies inside a hole sums to 0 out of integral values near
                    1000, so the four rounded corners leave a residue of either sign even where the window is inside the patch;
  one_subregion     a 2 x 2 blob at rows / columns 1 .. 2: at mrSize 20.5 (samples every 2 px from -3, Haar size 4) only the
                    samples k, l <= -9 see it, and those belong to the first sub-region alone.

MR_SIZES: 5.1962 the reference's default (scale 7.89: most of the window outside the patch); 20.5 (scale 2); 16.4 (scale 2.5:
k * scale ends in .5 for odd k, fRound(2.5) = 3); 30.0 (fRound(scale) = 1); 100.0 (fRound(scale) = 0: Haar size 0, NaN rows)."""
import functools

import numpy as np

import surf_model as M

L = M.L
MR_SIZES = (5.1962, 20.5, 16.4, 30.0, 100.0)
MR_NAN = (100.0,)                 # every row is NaN
INTEGRAL_OF = ("random_0", "region_0", "step_x", "bright_flat_0")        # the fixture records the integral image of these, in case order
N_REGIONS = 6


@functools.lru_cache(maxsize=None)
def _region_patches():
    from oracle import pyoracle as O
    from tests import describe_cases as DC
    regs = np.concatenate([DC.regions_of(P) for P in (25, 63)])[:N_REGIONS]
    out = []
    for i in range(len(regs)):
        p = O.extract_patch(DC.image(), regs[i:i + 1], mr_size=float(DC.MR_SIZE))
        out.append(O.describe_patch(p, photo_norm=1)[1].reshape(L, L))
    return out


@functools.lru_cache(maxsize=None)
def _build():
    out = []

    def add(name, p):
        p = np.ascontiguousarray(p, np.float32).reshape(L, L)
        assert np.isfinite(p).all()
        p.setflags(write=False)
        out.append((name, p))

    for s in range(10):
        add("random_%d" % s, np.random.default_rng(9000 + s).uniform(0.0, 255.0, (L, L)))
    for s in range(4):
        add("levels_%d" % s, np.random.default_rng(9100 + s).integers(0, 256, (L, L)))
    for s, p in enumerate(_region_patches()):
        add("region_%d" % s, p)
    add("constant", np.full((L, L), 128.5))
    add("zero", np.zeros((L, L)))
    add("saturated", np.full((L, L), 255.0))
    y, x = np.mgrid[0:L, 0:L]
    add("step_x", np.where(x < 20, 10.0, 240.0))
    add("step_y", np.where(y < 23, 240.0, 10.0))
    for name, (r, c) in (("pixel_tl", (0, 0)), ("pixel_tr", (0, L - 1)), ("pixel_bl", (L - 1, 0)), ("pixel_br", (L - 1, L - 1)),
                         ("pixel_centre", (20, 20))):
        p = np.zeros((L, L))
        p[r, c] = 255.0
        add(name, p)
    for s in range(6):
        add("bright_flat_%d" % s, 250.0 + np.random.default_rng(9200 + s).uniform(0.0, 1.0, (L, L)))
    for s in range(2):
        rng = np.random.default_rng(9300 + s)
        p = 250.0 + rng.uniform(0.0, 1.0, (L, L))
        for r, c in zip(rng.integers(8, 36, 40), rng.integers(8, 36, 40)):
            p[r:r + 3, c:c + 3] = 0.0
        add("bright_holes_%d" % s, p)
    blob = np.zeros((L, L))
    blob[1:3, 1:3] = 200.0
    add("one_subregion", blob)
    return tuple(out)


def cases():
    return list(_build())


def names():
    return [n for n, _ in _build()]


def patches():
    """[n][41][41] f32, in the order of cases()"""
    return np.stack([p for _, p in _build()])


_MODEL = {}


def model(mr_size):
    """[n][64] f32: surf_model.describe of patches() at mr_size, computed once per process; info(mr_size) goes with it"""
    if mr_size not in _MODEL:
        info = {}
        d = M.describe(patches(), mr_size, info=info)
        d.setflags(write=False)
        _MODEL[mr_size] = (d, info)
    return _MODEL[mr_size][0]


def info(mr_size):
    model(mr_size)
    return _MODEL[mr_size][1]
