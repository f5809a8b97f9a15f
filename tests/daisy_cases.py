"""The patches and parameter sets of the DAISY tests (tests/test_daisy_model_cpu.py, tests/test_gpu_daisy.py,
tools/make_daisy_fixture.py): 41 x 41 f32, from integer formulas, seeded numpy or the oracle's patch extraction, built once per
process and left alone.  cases() -> list of (name, patch).  What a name claims is checked against the model in
tests/test_daisy_model_cpu.py, never assumed.

Families:
  random_*        seeded uniform values in [0, 255], full mantissas (the byte conversion rounds them);
  levels_*        seeded integer grey levels 0 .. 255;
  region_*        the oracle's photonormalised patches of regions on describe_cases.image() (surf_cases: the same constructions);
  flat, zero      one value everywhere: every gradient and every norm is 0, nothing is divided, the row is all zeros;
  step_v          columns < 20 at 40, the rest at 200: NRM_SIFT clips at 0.154 and runs a second round, so it differs from NRM_FULL;
  step_h          the same across rows;
  textured_left   seeded levels left of column 12, 100 elsewhere: under NRM_PARTIAL some histograms are zero beside non-zero ones;
  half_even       values k + 0.5 for even and odd k (rint gives k or k + 1), mixed with k + 0.25 / k + 0.75;
  saturation      values from -60 to 330 with fractions: the byte conversion saturates at both ends;
  border_only     structure in rows and columns 0, 1, 39, 40 only, 128 inside: what the replicated borders carry inward;
  pixel_centre    one pixel of 255 on zeros.

PARAMS, (rad, radq, thq, histq): the reference's defaults; the shipped ini's rad = 20 (the +x and +y points of the outer ring sit
just below 40: zeroed); one ring at rad = 20 (sigma 10: 51 taps, the longest filter; the same two points sit at 40: skipped); a
small grid of 2 x 4; rad = 1 (the sigmas of the cubes give filter lengths at the floor of 3).  Each runs at the three normalisations."""
import functools

import numpy as np

import daisy_model as M

L = M.L
PARAMS = ((15, 3, 8, 8), (20, 3, 8, 8), (20, 1, 8, 8), (7, 2, 4, 8), (1, 3, 8, 8))
NRMS = (M.NRM_PARTIAL, M.NRM_FULL, M.NRM_SIFT)
PLANES_OF = ("random_0", "border_only")     # the fixture records blurred, dx, dy of these, in case order
CUBES_OF = "random_0"                        # and layer CUBE_LAYER of every cube of this one, per parameter set
CUBE_LAYER = 3
N_REGIONS = 4


@functools.lru_cache(maxsize=None)
def _build():
    import surf_cases
    out = []

    def add(name, p):
        p = np.ascontiguousarray(p, np.float32).reshape(L, L)
        assert np.isfinite(p).all()
        p.setflags(write=False)
        out.append((name, p))

    for s in range(4):
        add("random_%d" % s, np.random.default_rng(9400 + s).uniform(0.0, 255.0, (L, L)))
    for s in range(2):
        add("levels_%d" % s, np.random.default_rng(9500 + s).integers(0, 256, (L, L)))
    for s, p in enumerate(surf_cases._region_patches()[:N_REGIONS]):
        add("region_%d" % s, p)
    y, x = np.mgrid[0:L, 0:L]
    add("flat", np.full((L, L), 128.0))
    add("zero", np.zeros((L, L)))
    add("step_v", np.where(x < 20, 40.0, 200.0))
    add("step_h", np.where(y < 23, 200.0, 40.0))
    add("textured_left", np.where(x < 12, np.random.default_rng(9600).integers(0, 256, (L, L)), 100))
    k = (7 * y + 3 * x) % 250
    add("half_even", k + np.choose((x + y) % 4, [0.5, 0.5, 0.25, 0.75]))
    add("saturation", -60.0 + ((13 * y + 29 * x) % 391) + np.random.default_rng(9700).uniform(0.0, 1.0, (L, L)))
    edge = (np.minimum(x, L - 1 - x) < 2) | (np.minimum(y, L - 1 - y) < 2)
    add("border_only", np.where(edge, np.random.default_rng(9800).integers(0, 256, (L, L)), 128))
    p = np.zeros((L, L))
    p[20, 20] = 255.0
    add("pixel_centre", p)
    return tuple(out)


def cases():
    return list(_build())


def names():
    return [n for n, _ in _build()]


def patches():
    """[n][41][41] f32, in the order of cases()"""
    return np.stack([p for _, p in _build()])


_MODEL = {}


def model(params, nrm_type):
    """[n][dim] f32: daisy_model.describe of patches() at params = (rad, radq, thq, histq), computed once per process"""
    key = (tuple(params), nrm_type)
    if key not in _MODEL:
        if (tuple(params), "raw") not in _MODEL:
            info = {}
            M.describe(patches(), *params, nrm_type=M.NRM_FULL, info=info)
            _MODEL[(tuple(params), "raw")] = info
        info = dict(_MODEL[(tuple(params), "raw")])
        d = M.normalize(info["raw"], nrm_type, info=info)
        d.setflags(write=False)
        _MODEL[key] = (d, info)
    return _MODEL[key][0]


def info(params, nrm_type):
    model(params, nrm_type)
    return _MODEL[(tuple(params), nrm_type)][1]
