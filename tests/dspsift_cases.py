"""The inputs of the DSP-SIFT tests (tests/test_dspsift_model_cpu.py, tests/test_gpu_dspsift.py, tools/make_dspsift_fixture.py),
built once per process and left alone.

Patches (patches(): [n][41][41] f32, names in patch_names()): the 54 of tests/liop_cases.py -- full mantissas, plateaus, clamped
photonormalised windows, subnormal and negative values -- and the oracle's photonormalised patches of raw_regions() on
describe_cases.image().

Norm rows (norm_rows(): list of (name, row [128] f32); what a name claims is checked against the model in
tests/test_dspsift_model_cpu.py, never assumed):
  zero               a row of zeros: len = 0, fac = inf, NaN values, zeros out;
  one_bin            one nonzero bin: it normalises to 1, clips, and the row is normalised again;
  flat               128 equal values, 1 / sqrt(128) each: nothing clips;
  exactly_0p2f       25 ones: every value normalises to (float)0.2, which maxBinValue = 0.2 clips and (double)0.2f does not;
  half_lo_* / half_hi_*   pairs of rows that differ by one f32 ulp in one bin, found by bisection over that bin's bit pattern:
                     512 v of the bin lands within one f32 ulp of b + 0.5, below it in _lo and at or above it in _hi;
  subnormal_all      every entry subnormal or 0: the squares underflow to 0, len = 0, the nonzero entries become inf and clip,
                     the zeros become NaN, the second length is NaN: zeros out;
  subnormal_dense    the same without zeros: every entry becomes inf, clips to (float)0.2, and the row comes out flat;
  subnormal_some     subnormal entries beside normal ones;
  tiny_squares       entries around 1e-20 whose squares are subnormal: the length is the root of a subnormal sum;
  wide_range         group sums spread over 20 binades: the serial f32 chain gives another length in another order;
  hist_* / pooled_*  raw histograms of case patches and sums of several."""
import functools

import numpy as np

import dspsift_model as M
import liop_cases as LC
from tests import describe_cases as DC

f32 = np.float32

# ---------------------------------------------------------------------------------------------------------------- regions
# raw histograms: one window size per path class of the planner and both sides of the direct-branch boundary (P = 0: s = 7, the
# direct branch; P = 19: s = 8), at describe_cases.MR_SIZE
RAW_SIZES = tuple(DC.CLASS_SIZE[c] for c in DC.CLASSES) + (0, 19)
# DSP-SIFT: numScales, startCoef, endCoef -- config_iter_cviu.ini's two equal scales, DomainSizePolingParams' defaults, and
# config_iter_extract_regs_photonorm.ini's sixteen
CONFIGS = ((1, 1.0, 1.0), (3, 0.5, 1.5), (15, 0.4, 1.35))
# the configurations the reference's files and defaults name (the mrSize_k test): the three above and config_iter_mods_cviu.ini's
NAMED_CONFIGS = CONFIGS + ((10, 0.5, 2.0),)
DSP_SIZES = (19, 25, 39, 47, 63, 77)       # interior, top-left and bottom-right region of each, and of the direct branch
DSP_DIRECT_S = 4.5                         # ceil(4.5 * 1.5) = 7: the direct branch at every coefficient up to 1.5
DSP_EXTRA_S = (9.0, 14.5, 20.0, 26.0, 31.0)   # two more centres at scales between those
FAST_S = 4.0                               # s * mrSize_k = 2, 3, 4 at coefs 0.5 .. 1.0 in two steps: integers, all direct
FAST_CONFIG = (2, 0.5, 1.0)


def _regions_of(P):
    return DC.regions_of(P) if P < 400 else DC.regions_of(P, which=(0,))     # the large windows: the interior region only


@functools.lru_cache(maxsize=None)
def raw_regions():
    regs = np.concatenate([_regions_of(P) for P in RAW_SIZES])
    regs["id"] = np.arange(len(regs))
    regs.setflags(write=False)
    return regs


@functools.lru_cache(maxsize=None)
def dsp_regions():
    """31 regions: windows of 19 .. 77 px at coefficient 1 (several planner classes; the small ones fall into the direct branch at
    the small coefficients), three that are direct at every scale, ten between"""
    parts = [DC.regions_of(P) for P in DSP_SIZES]
    parts.append(DC.make_regions([(DC.CENTRES[w][0], DC.CENTRES[w][1], DC.shape_of(19, w == 0), DSP_DIRECT_S) for w in (0, 1, 2)]))
    parts.append(DC.make_regions([(DC.CENTRES[w][0], DC.CENTRES[w][1], DC.shape_of(int(2 * s + 3), False), s)
                                  for s in DSP_EXTRA_S for w in (3, 4)]))
    regs = np.concatenate(parts)
    regs["id"] = np.arange(len(regs))
    regs.setflags(write=False)
    return regs


@functools.lru_cache(maxsize=None)
def fast_regions():
    regs = DC.make_regions([(DC.CENTRES[w][0], DC.CENTRES[w][1], DC.shape_of(19, w == 0), FAST_S) for w in (0, 1, 2, 3)])
    regs.setflags(write=False)
    return regs


@functools.lru_cache(maxsize=None)
def chunk_regions():
    """60 regions with windows of 315 px at coefficient 1: 5.9 M floats of windows, more than a 16 MiB arena (4 M) holds; at
    coefficient 1.5 four times that arena, at 0.5 less than one"""
    regs = np.concatenate([DC.regions_of(315) for _ in range(20)])
    regs["id"] = np.arange(len(regs))
    regs.setflags(write=False)
    return regs


CHUNK_CONFIG = (3, 0.5, 1.5)


def oracle_patch(img, reg, mr_size, photo_norm):
    """the patch DescribeRegions<> hands to its functor for one region (the accurate branch), from the oracle"""
    from oracle import pyoracle as O
    p = O.extract_patch(img, reg, mr_size=float(mr_size))
    return O.describe_patch(p, photo_norm=1)[1].reshape(41, 41) if photo_norm else p


# ---------------------------------------------------------------------------------------------------------------- patches
@functools.lru_cache(maxsize=None)
def _patches():
    names = ["liop_" + n for n, _ in LC.cases()]
    pats = [p for _, p in LC.cases()]
    regs = raw_regions()
    for i in range(len(regs)):
        names.append("region_%d" % i)
        pats.append(oracle_patch(DC.image(), regs[i:i + 1], DC.MR_SIZE, 1))
    out = np.stack(pats).astype(f32)
    out.setflags(write=False)
    return tuple(names), out


def patch_names():
    return list(_patches()[0])


def patches():
    return _patches()[1]


@functools.lru_cache(maxsize=None)
def model_raw():
    """[n][128] f32: the model's raw histograms of patches()"""
    out = np.stack([M.raw(p) for p in patches()])
    out.setflags(write=False)
    return out


# -------------------------------------------------------------------------------------------------------------- norm rows
MAX_BINS = (0.2, float(f32(0.2)))          # the ini's 0.2 and SIFTDescriptorParams' own default, maxBinValue = 0.2f


def _bits(x):
    return int(np.asarray(x, f32).view(np.uint32))


def _from_bits(b):
    return np.asarray(b, np.uint32).view(f32)[()]


def _half_pair_of(seed, bin_, max_bin=0.2):
    """two rows that differ by one ulp in `bin_`, whose output in that bin differs by one: a random non-clipping row in which the
    bin's value is bisected over its bit patterns"""
    rng = np.random.default_rng(seed)
    row = rng.uniform(0.5, 1.0, 128).astype(f32)

    def out_of(bits):
        r = row.copy()
        r[bin_] = _from_bits(bits)
        return int(M.sift_norm_f32(r, max_bin)[bin_])

    lo, hi = _bits(f32(0.5)), _bits(f32(1.0))
    assert out_of(lo) < out_of(hi)
    target = out_of(lo)
    while hi - lo > 1:                        # out_of(lo) == target < out_of(hi) throughout
        mid = (lo + hi) // 2
        if out_of(mid) == target:
            lo = mid
        else:
            hi = mid
    a, b = row.copy(), row.copy()
    a[bin_], b[bin_] = _from_bits(lo), _from_bits(hi)
    return a, b


def _half_pair(seed, bin_, max_bin=0.2):
    """the first pair of seeds seed, seed + 1, .. in which 512 v of the bin lies within one f32 ulp of b + 0.5 in both rows (the
    bisection alone guarantees the flip; the two values may lie up to two ulps apart)"""
    for sd in range(seed, seed + 100):
        a, b = _half_pair_of(sd, bin_, max_bin)
        info = {}
        out = M.sift_norm_f32(np.stack([a, b]), max_bin, info=info)
        half = float(out[0][bin_]) + 0.5
        ulp = float(np.spacing(f32(half)))
        va, vb = float(info["t"][0][bin_]) - 0.5, float(info["t"][1][bin_]) - 0.5
        if not info["clipped"].any() and 0 < half - va <= ulp and 0 <= vb - half <= ulp:
            return a, b
    raise AssertionError("no ulp pair found")


@functools.lru_cache(maxsize=None)
def _norm_rows():
    out = []
    out.append(("zero", np.zeros(128, f32)))
    one = np.zeros(128, f32)
    one[37] = f32(3.25)
    out.append(("one_bin", one))
    out.append(("flat", np.full(128, f32(7.5), f32)))
    exact = np.zeros(128, f32)
    exact[3::5] = f32(1.0)                    # 25 ones: len = 5, every value (float)0.2 -- above 0.2, not above (double)0.2f
    assert int(exact.sum()) == 25
    out.append(("exactly_0p2f", exact))
    for k, (seed, bin_) in enumerate(((1100, 5), (1200, 64), (1300, 127))):
        a, b = _half_pair(seed, bin_)
        out.append(("half_lo_%d" % k, a))
        out.append(("half_hi_%d" % k, b))
    rng = np.random.default_rng(77)
    sub = (rng.integers(0, 1 << 23, 128).astype(np.uint32)).view(f32).copy()     # exponent field 0: subnormal (or 0)
    sub[::9] = 0
    out.append(("subnormal_all", sub))
    out.append(("subnormal_dense", np.where(sub == 0, _from_bits(1), sub).astype(f32)))
    some = rng.uniform(0.0, 3.0, 128).astype(f32)
    some[::3] = sub[::3]
    out.append(("subnormal_some", some))
    out.append(("tiny_squares", (rng.uniform(0.5, 2.0, 128) * 1e-20).astype(f32)))
    out.append(("wide_range", (rng.uniform(1.0, 2.0, 128) * np.exp2(rng.integers(-10, 11, 128).astype(np.float64))).astype(f32)))
    raw = model_raw()
    names = patch_names()
    for i in range(0, len(raw), 2):
        out.append(("hist_" + names[i], raw[i]))
    for i in range(0, len(raw) - 4, 5):
        out.append(("pooled_%d" % i, M.pool(raw[i:i + 4])))
    for _, r in out:
        r.setflags(write=False)
    return tuple(out)


def norm_rows():
    return list(_norm_rows())


def norm_row_array():
    return np.stack([r for _, r in _norm_rows()])
