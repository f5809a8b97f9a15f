"""GPU: LIOP, SURF, DAISY and extract_patches share one patch buffer and one staging buffer per context (engine_patchdesc.hip).
Interleaved on one context, in an order that makes both buffers grow and then serve a smaller user of another row width, every
call returns the bytes it returns on a context of its own, and every descriptor's counters show its own calls and no others."""
import numpy as np
import pytest

import liop_cases as LC
import surf_cases as SC
from test_gpu_daisy import daisy_regions                    # noqa: F401  (fixtures of the neighbouring modules)
from test_gpu_liop import liop_regions, patch_regions       # noqa: F401
from test_gpu_surf import image, surf_regions               # noqa: F401
from tests import describe_cases as DC

pytestmark = pytest.mark.gpu

MR = DC.MR_SIZE
SURF_MR = 20.5                 # scale 2: finite rows on the case patches


def test_interleaved_calls_match_fresh_contexts(modsx, image, surf_regions, daisy_regions, liop_regions):     # noqa: F811
    assert len(surf_regions) == len(daisy_regions) == len(liop_regions) == 9
    big, small = dict(rad=15, radq=3, thq=8), dict(rad=15, radq=1, thq=4)
    # (call, bytes of patchBuf it needs, bytes of patchOut it needs)
    steps = [
        (lambda c: c.extract_patches(image, liop_regions[:3], mr_size=MR), 0, 3 * 1681 * 4),
        (lambda c: c.describe_regions_surf(image, surf_regions, mr_size=MR), 9 * 1681 * 4, 9 * 64 * 4),
        (lambda c: c.liop_patches(LC.patches()[:5]), 5 * 1681 * 4, 5 * 144 * 4),
        (lambda c: c.describe_regions_daisy(image, daisy_regions, mr_size=MR, **big), 9 * 1681 * 4, 9 * 200 * 4),
        (lambda c: c.describe_regions_daisy(image, daisy_regions, mr_size=MR, **small), 9 * 1681 * 4, 9 * 40 * 4),
        (lambda c: c.describe_regions_liop(image, liop_regions[:3], mr_size=MR), 3 * 1681 * 4, 3 * 144 * 4),
        (lambda c: c.surf_patches(SC.patches()[:5], mr_size=SURF_MR), 5 * 1681 * 4, 5 * 64 * 4),
        (lambda c: c.extract_patches(image, liop_regions, mr_size=MR), 0, 9 * 1681 * 4),
    ]
    # the order does what the module is about: each buffer is (re)allocated at some step and a later step asks it for less
    for k in (1, 2):
        need = [s[k] for s in steps]
        grows = [i for i in range(len(need)) if need[i] > max([0] + need[:i])]
        assert any(0 < need[j] < need[i] for i in grows for j in range(i + 1, len(need))), need
    assert steps[-1][2] > max(s[2] for s in steps[:-1])        # and the staging buffer is reallocated after seven users

    shared = modsx.Context(0)
    try:
        got = [call(shared) for call, _, _ in steps]
        counters = shared.liop_counters(), shared.surf_counters(), shared.daisy_counters()
    finally:
        shared.close()
    want, exact = [], 0
    for call, _, _ in steps:
        fresh = modsx.Context(0)
        try:
            want.append(call(fresh))
            exact += fresh.liop_counters()["exact_path"]
        finally:
            fresh.close()
    shapes = [(3, 41, 41), (9, 64), (5, 144), (9, 200), (9, 40), (3, 144), (5, 64), (9, 41, 41)]
    for i, (g, w, shape) in enumerate(zip(got, want, shapes)):
        assert g.shape == w.shape == shape and g.dtype == w.dtype == np.float32, (i, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), "step %d differs from the same call on a fresh context" % (i + 1)
    liop, surf, daisy = counters
    assert liop == dict(calls=2, regions=5 + 3, exact_path=exact, sub_batches=2), liop
    assert surf == dict(calls=2, patches=9 + 5, sub_batches=2), surf
    assert daisy == dict(calls=2, patches=9 + 9, sub_batches=2), daisy
