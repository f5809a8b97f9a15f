"""GPU: tiles of every shape in ONE launch of the LDS describe kernels, against the oracle.

tests/test_gpu_describe_paths.py describes every window size in a call of its own, so a launch of k_sample_rows_lds there holds
tiles of one shape.  Which lane takes which sample or output pair depends on the tile (mods_amd/csrc/describe_lanes.hpp: the
columns a wavefront parks follow its row count, the slots a wavefront runs in the last filter round follow the pair count), so
here one Context.describe_regions call mixes the sizes: 15 window sizes from the fused small-window path to P = 349 (row tiles
of 5 rows), three regions each (two of P = 19) -- interior (no-border sampling), top-left and bottom-right (border path) -- in an order that
puts different sizes next to each other.  A second call runs the same list reversed with one region dropped (an odd count).
Both must equal the oracle's rows exactly (tests/describe_cases.py: image, regions_of, references -> oracle_rows).
"""
import numpy as np
import pytest

from tests import describe_cases as DC

pytestmark = pytest.mark.gpu

SIZES = (19, 29, 33, 35, 43, 45, 47, 63, 67, 77, 101, 135, 151, 203, 349)


def _order():
    """(P, region) of the mixed list: small and large sizes alternate, and the three regions of a size lie 15 places apart"""
    lo, hi = SIZES[:8], SIZES[8:][::-1]
    mixed = [p for pair in zip(lo, hi + (None,)) for p in pair if p is not None]
    assert sorted(mixed) == sorted(SIZES)
    order = [(P, w) for w in (0, 1, 2) for P in (mixed if w != 1 else mixed[::2] + mixed[1::2])]
    order.remove((19, 2))          # 44 regions, so that the second call, one fewer, has an odd count
    return order


@pytest.fixture(scope="module")
def mixed():
    order = _order()
    refs = DC.references(SIZES)
    regs = np.concatenate([DC.regions_of(P, which=(w,)) for P, w in order])
    want = np.stack([refs[P][w] for P, w in order])
    assert len(regs) == 44 and all(order[i][0] != order[i + 1][0] for i in range(len(order) - 1))
    return regs, want


def _check(got, want, order):
    bad = ["%d: P = %d region %d: %d of 128 entries differ" % (i, P, w, int((got[i] != want[i]).sum()))
           for i, (P, w) in enumerate(order) if not np.array_equal(got[i], want[i])]
    assert not bad, "\n".join(bad)
    assert np.array_equal(got, want)


def test_mixed_sizes_in_one_call_equal_oracle(ctx, modsx, mixed):
    regs, want = mixed
    im = ctx.upload(DC.image())
    try:
        c0 = ctx.describe_counters()
        got = ctx.describe_regions(im, regs.view(modsx.REGION), mr_size=DC.MR_SIZE)
        c1 = ctx.describe_counters()
        assert (c1["calls"] - c0["calls"], c1["chunks"] - c0["chunks"], c1["jobs"] - c0["jobs"]) == (1, 1, 44)
        assert c1["fused_windows"] > c0["fused_windows"] and c1["lds_col_tiles"] > c0["lds_col_tiles"]
        assert c1["global_row_tiles"] == c0["global_row_tiles"]          # every window here takes the LDS kernels
        _check(got, want, _order())
    finally:
        im.free()


def test_reversed_odd_count_equals_oracle(ctx, modsx, mixed):
    regs, want = mixed
    keep = [i for i in range(len(regs)) if i != 17][::-1]
    order = [_order()[i] for i in keep]
    im = ctx.upload(DC.image())
    try:
        got = ctx.describe_regions(im, np.ascontiguousarray(regs[keep]).view(modsx.REGION), mr_size=DC.MR_SIZE)
        assert len(got) == 43
        _check(got, want[keep], order)
    finally:
        im.free()
