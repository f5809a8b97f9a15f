"""Inputs of the SIFT histogram parity tests (tests/test_sift_patch_cases_cpu.py proves the claims, tests/test_gpu_sift_patches.py
runs them through Context.describe_regions / describe_regions_raw / extract_patches).  No GPU in here.

The identity harness: a region with A = I, an integer centre and s * mr_size = 20 (s = 1, mr_size = 20), described with fast = 1,
takes k_describe's direct branch with unit step and zero bilinear weights: the kernel's 41 x 41 patch is
img[y - 20 : y + 21, x - 20 : x + 21] bit for bit (the CPU test shows it on the oracle: describe_regions on the composed image ==
describe_patch on every patch, also at s = 2, mr_size = 10).  The bilinear tap still multiplies column x + 21 and row y + 21 by a
weight of 0, so `compose()` keeps one blank column and at least one blank row behind every cell; no pixel is non-finite (the
overflow case overflows in the kernel's xg * xg, from finite pixels).

Which two regions share a workgroup (describe_plan.cpp: sort_jobs, kernels_describe.hip: k_describe): the regions of a call (one
chunk: direct-branch regions take no window arena) are stably sorted by (image, (int)y >> 6, (int)x), and workgroup w takes the
regions 2 w and 2 w + 1 of that order; the last region of an odd call is its own partner.  A workgroup takes the ordered gather
when either of its regions needs it.  `launch_order`, `workgroups` and `predicted_ordered` state that rule; the GPU test lets the
`ordered_workgroups` counter confirm it.  `compose()` gives every row of cells its own 64-row band, so that x alone orders a row:
  blank  case  blank  case  ...  blank        (pitch 42 px; a blank cell is a region of zeros, the FORCER)
A region of zeros is not scalable (mxb == 0) under either photo_norm, so a case listed with the blank cell to its right (arrangement
2: case in slot 0) or to its left (arrangement 3: case in slot 1) goes through the ordered gather whatever it needs on its own.

Planted patches (`planted()`; every record: name, family, patch [41, 41] f32, options = OPTIONS[family], claim).  claim["inexact"]
maps photo_norm -> the trigger that sends the region to the ordered gather on its own (one of sift_gather_model.TRIGGERS) or None
(order-free); records without it are proven order-free / ordered by the model alone, which the counter then confirms.
  ramps        orient_cases' ramps, photo_norm = 0: the 8 sign / octant codes x table index 0 .. 255 of atan2lut_case and the
               special entry 2048, index 255 by its rounded quotient, x == 0, exactly pi and exactly -pi; plus the uniform ramp that
               comes nearest to a bin of 2^53 after scaling (it cannot get there: sift_gather_model's docstring, BIG_BIN_REACHED)
  photometric  flat (var = 0: not normalised, no votes); a pair one ulp apart in one pixel whose (double)var lies just below and
               at / above 0.0001; clamps at 0 and at 255; mean 1e6 with small variation (the f32 running sum rounds at almost
               every add); negative values.  Each under photo_norm 0 and 1.
  gather       (a) ordinary, (b) a pixel pair one ulp apart next to a strong gradient: smallest scaled term below 2^23, (d) a region
               of zeros, (e) gradient products that are all subnormal (E < -60).  (c), a bin at 2^53, is unreachable.
  magnitude    one smooth patch times powers of two: E = -70, -61, -60, -59, 0, 47, 48, 63; a bump with E = 64 (the largest a finite
               |grad| allows); and the smooth patch past the overflow of xg * xg (|grad| = inf, NaN where the mask is 0).
               E_REACHABLE / VAL_REACHABLE: what the model finds over every power of two, all the arithmetic allows.
  norm         one nonzero gradient pixel (a frame site: 4 bins, the largest clips at max_bin, renormalised); an all-zero histogram
               (length 0, NaN -> 0); patches whose 512 v + 0.5 lies within one f64 ulp of an integer, below and at / above it
               (`_rounding_cases`, NORM_SEARCH_COUNT per side and descriptor type).  Under all four descriptor types.
  random       RANDOM_PER_KIND each of smooth, white, low-contrast and integer-quantised noise, and liop_cases' 54 patches.
"""
import numpy as np

import dspsift_model as D
import liop_cases as LC
import orient_cases as OC
import sift_gather_model as G

F = np.float32
PS, HALF = 41, 20
MR_SIZE, FAST = 20.0, 1
PITCH_X, PITCH_Y, X0, Y0 = 42, 64, 24, 32
PER_ROW, ROWS_PER_IMAGE = 16, 11            # 176 cases and 1393 x 704 px (3.9 MB) per image at the most
RANDOM_PER_KIND = 24
NORM_SEARCH_COUNT = 8
OPTIONS = {
    "ramps": dict(photo_norm=(0,), desc_types=(0, 1)),
    "photometric": dict(photo_norm=(0, 1), desc_types=(1,)),
    "gather": dict(photo_norm=(0,), desc_types=(0, 1)),
    "magnitude": dict(photo_norm=(0,), desc_types=(0, 1)),
    "norm": dict(photo_norm=(0,), desc_types=(0, 1, 2, 3)),
    "random": dict(photo_norm=(0, 1), desc_types=(1, 3)),
}
GROUPS = (("ramps",), ("photometric",), ("gather", "magnitude"), ("norm",), ("random",))     # families that share an image set
IMAGES_PER_GROUP = (12, 1, 1, 1, 1)         # what images() makes of them (fixed here so that collecting the GPU tests builds nothing)
N_IMAGES = sum(IMAGES_PER_GROUP)
# established by test_sift_patch_cases_cpu.py::test_magnitude_and_reachable_range from the model, over every power of two (times 1, 1.5 and the
# largest mantissa) of the magnitude family's base patch and of a bump next to the centre and next to the mask's smallest pixel;
# it is all the arithmetic allows (sift_gather_model's docstring).  k_describe's `scalable` accepts E in [-60, 64].
E_REACHABLE = (-76, 64)
VAL_REACHABLE = (2.0 ** -77, 2.0 ** 64)      # a nonzero finite val lies in [lo, hi)
MAGNITUDE_E = (-70, -61, -60, -59, 0, 47, 48, 63)      # 63: the largest for the smooth base; 64: magnitude/E+64_bump
BIG_BIN_REACHED = (0.8, 0.9)                 # largest X / 2^53 of sift/ramp/big_bin_candidate lies in between

_planted = None


def _smooth_base(seed, amp=60.0, passes=2):
    rs = np.random.RandomState(seed)
    return OC._smooth(rs.standard_normal((PS, PS)).astype(F) * F(amp), passes)


def _rec(name, family, patch, **claim):
    return dict(name=name, family=family, patch=np.ascontiguousarray(patch, F), options=OPTIONS[family], claim=claim)


def _ramps():
    out = [_rec("sift/" + c["name"], "ramps", c["patch"], **{k: v for k, v in c["claim"].items() if k in ("entry", "special")})
           for c in OC.planted() if c["family"] == "ramps"]
    # angle 0 (o == 8 exactly: one orientation bin takes the whole vote), |grad| = 1.9375 just under 2^1, mask 1 at the centre
    out.append(_rec("sift/ramp/big_bin_candidate", "ramps", OC.ramp(1.9375, 0.0), entry=(5, 0), big_bin_candidate=True))
    return out


def var_below(patch):
    return bool(np.float64(G.photo_stats(patch)[1]) < 0.0001)


def _var_pair():
    """two patches, zero but for pixel (20, 20), one ulp apart there: (double)var < 0.0001 for the first and not for the second"""
    def patch(bits):
        p = np.zeros((PS, PS), F)
        p[20, 20] = np.array([bits], np.uint32).view(F)[0]
        return p
    lo, hi = int(np.array([1e-3], F).view(np.uint32)[0]), int(np.array([1e-2], F).view(np.uint32)[0])
    assert var_below(patch(lo)) and not var_below(patch(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if var_below(patch(mid)):
            lo = mid
        else:
            hi = mid
    return patch(lo), patch(hi)


def _photometric():
    rs = np.random.RandomState(4101)
    lo, hi = _var_pair()
    white = (rs.standard_normal((PS, PS)) * 40).astype(F)
    offset = F(1e6) + (rs.randint(-64, 65, (PS, PS)) / 16.0).astype(F)          # ulp(1e6) = 1/16: every pixel is exact
    return [_rec("photo/flat", "photometric", np.full((PS, PS), 90.0, F), inexact={0: "not_scalable", 1: "not_scalable"}, normalised=False),
            _rec("photo/var_below", "photometric", lo, normalised=False, var_pair="below"),
            _rec("photo/var_at_or_above", "photometric", hi, normalised=True, var_pair="above"),
            _rec("photo/clamp_both", "photometric", white, normalised=True, clamps=(0.0, 255.0)),
            _rec("photo/large_offset", "photometric", offset, normalised=True, rounding_adds=True),
            _rec("photo/negative", "photometric", _smooth_base(4102) - F(300.0), normalised=True)]


def _gather():
    small = np.zeros((PS, PS), F)
    small[20, 20] = 1000.0                                   # the strong gradient: max val about 2^10
    small[10, 10], small[10, 12] = 1.0, np.nextafter(F(1.0), F(2.0))      # pixel (10, 11): xg = 2^-23, yg = 0
    tiny = (_smooth_base(4201).astype(np.float64) * 2.0 ** -76).astype(F)
    return [_rec("gather/ordinary", "gather", _smooth_base(4200) + F(20), inexact={0: None}),
            _rec("gather/small_term", "gather", small, inexact={0: "small_term"}),
            _rec("gather/zeros", "gather", np.zeros((PS, PS), F), inexact={0: "not_scalable"}),
            _rec("gather/subnormal_products", "gather", tiny, inexact={0: "not_scalable"}, subnormal_products=True)]


def magnitude_base():
    return _smooth_base(4300)


def scaled(base, e_from, e_to):
    return (base.astype(np.float64) * 2.0 ** (e_to - e_from)).astype(F)


def _magnitude():
    base = magnitude_base()
    e0 = G.decide(base)["E"]
    out = [_rec("magnitude/E%+03d" % e, "magnitude", scaled(base, e0, e), E=e,
                inexact={0: None if G.E_MIN <= e <= G.E_MAX else "not_scalable"}) for e in MAGNITUDE_E]
    bump = np.zeros((PS, PS), F)
    bump[20, 21] = np.nextafter(F(2.0 ** 64), F(0))         # pixel (20, 20): xg just under 2^64 (its square is finite), mask 1
    out.append(_rec("magnitude/E+64_bump", "magnitude", bump, E=64, inexact={0: None}))
    out.append(_rec("magnitude/overflow", "magnitude", scaled(base, e0, 72), inexact={0: "not_scalable"}, overflow=True))
    return out


def norm_t_batch(H, desc_type, max_bin=0.2):
    """dspsift_model.describe_f64 up to the truncation, on rows [n][128]: t = 512 v + 0.5 in f64 (NaN where the norm was 0),
    [n][128] or [n][64].  The same statements in the same order, one histogram per row."""
    v = np.asarray(H, np.float64).reshape(-1, D.DIM).copy()
    if desc_type >= 2:
        v = (v.reshape(-1, 16, 2, 4)[:, :, 0] + v.reshape(-1, 16, 2, 4)[:, :, 1]).reshape(len(v), -1)

    def normalize(v):
        ln = np.zeros(len(v))
        for i in range(0, v.shape[1], 4):
            ln = ln + (((v[:, i] * v[:, i] + v[:, i + 1] * v[:, i + 1]) + v[:, i + 2] * v[:, i + 2]) + v[:, i + 3] * v[:, i + 3])
        return v * (np.float64(1.0) / np.sqrt(ln))[:, None]

    with np.errstate(all="ignore"):
        v = normalize(v)
        over = v > np.float64(max_bin)
        ch = over.any(1)
        if ch.any():
            v[ch] = normalize(np.where(over[ch], np.float64(max_bin), v[ch]))
        if desc_type & 1:
            s = np.zeros(len(v))
            for i in range(v.shape[1]):
                s = s + np.abs(v[:, i])
            return np.float64(512.0) * np.sqrt(v / s[:, None]) + 0.5
        return np.float64(F(512.0)) * v + 0.5


def norm_t(vec, desc_type, max_bin=0.2):
    return norm_t_batch(np.asarray(vec, np.float64)[None], desc_type, max_bin)[0]


def _norm():
    single = np.zeros((PS, PS), F)
    single[20, 0] = 8.0                       # a frame pixel: only (20, 1) gets a gradient under the mask
    return [_rec("norm/single_pixel", "norm", single, live=1, clipped=True, inexact={0: None}),
            _rec("norm/zero_histogram", "norm", np.full((PS, PS), 7.0, F), live=0, inexact={0: "not_scalable"})] + _rounding_cases()


# ---- the rounding search ---------------------------------------------------------------------------------------------------------
# A base patch whose rows 36 .. 40 are zero, one interior pixel V and three frame pixels (40, 18), (40, 20), (40, 22): a frame pixel
# gives pixel (39, c) the gradient (0, P) and nothing else under the mask, and row 39 is the last masked row, so the three
# sites' terms are the LAST adds of their bins (106 and 114), in column order.  t_i = 512 v_i + 0.5 of a target bin i moves with V
# by whole units, with the sites through the norm alone: by 1e-2, 1e-5 and 1e-8 over their ranges and by less than an f64 ulp
# of t per f32 step of the last one.  Four bisections over the knobs' bit patterns, each between two values on opposite sides of
# an integer N, end at two patches one f32 ulp apart in one pixel with t_i just below N and at / above it.
ROUND_SITES = ((40, 18), (40, 20), (40, 22))            # knobs A, C, B in raster order
ROUND_V = (12, 20)
ROUND_RANGES = dict(A=(1.0, 300.0), B=(1e-3, 0.3), C=(1e-7, 1e-4))


def _bits_of(x):
    return int(np.array([x], F).view(np.uint32)[0])


def _float_of(b):
    return np.array([b], np.uint32).view(F)[0]


def _rounding_base():
    base = (_smooth_base(4400) + F(20)).copy()
    base[36:, :] = 0
    return base


def _site_terms(P, col):
    """the two nonzero terms (bins 106, 114) of frame-site value(s) P > 0 at column col, f64 [n, 2]: samplePatch's f32 products"""
    P = np.atleast_1d(np.asarray(P, F))
    _, _, w0, w1 = D.bins_and_weights()
    val = (D.mask()[39, col] * np.sqrt(P * P)).astype(F)
    wr0 = F(w0[39])
    wc0, wc1 = (w0[col] * val.astype(np.float64)).astype(F), (w1[col] * val.astype(np.float64)).astype(F)
    o = G.o_table()[2 * 256]                                  # x == 0, y > 0: angle pi / 2, o = 10
    wo0 = F(1.0) - (o - F(int(o)))
    return np.stack([((wr0 * wc0) * wo0).astype(np.float64), ((wr0 * wc1) * wo0).astype(np.float64)], 1)


def _rounding_hist(base_hist, A, C, B):
    n = max(np.size(A), np.size(C), np.size(B))
    H = np.repeat(np.asarray(base_hist, np.float64)[None], n, 0)
    for P, col in ((A, 18), (C, 20), (B, 22)):
        t = _site_terms(np.broadcast_to(np.asarray(P, F), (n,)), col)
        H[:, 106] = H[:, 106] + t[:, 0]
        H[:, 114] = H[:, 114] + t[:, 1]
    return H


def _rounding_patch(base, V, A, C, B):
    p = base.copy()
    p[ROUND_V] = V
    for (r, c), P in zip(ROUND_SITES, (A, C, B)):
        p[r, c] = P
    return p


def _bisect(pred, lo, hi):
    """bit patterns lo < hi with pred(lo) != pred(hi) -> adjacent patterns with that property"""
    plo = pred(lo)
    assert plo != pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid) == plo:
            lo = mid
        else:
            hi = mid
    return lo, hi


def _rounding_cases():
    base = _rounding_base()
    mid = {k: F(np.sqrt(a * b)) for k, (a, b) in ROUND_RANGES.items()}
    v0 = float(base[ROUND_V])
    vs = [F(v0 + d) for d in (-120, -80, -40, 0, 40, 80, 120)]
    out = []

    def base_hist(V):
        d = G.decide(_rounding_patch(base, V, 0, 0, 0))
        assert not d["inexact"]                    # order-free: ldexp(X, E - 47) IS the reference's histogram
        return d["order_free"]

    hists = [base_hist(V) for V in vs]
    for dt in range(4):
        tv = np.stack([norm_t_batch(_rounding_hist(h, mid["A"], mid["C"], mid["B"]), dt)[0] for h in hists])      # [7, dim]
        skip = {106, 114} if dt < 2 else {106 - 52, 114 - 56, 106 - 56, 114 - 60}
        cand = [i for i in np.argsort(-tv[3]) if i not in skip and 8 < tv[3][i] < 100]
        found = 0
        for i in cand:
            if found == NORM_SEARCH_COUNT:
                break
            k = next((k for k in range(6) if int(tv[k][i]) != int(tv[k + 1][i])), None)
            if k is None:
                continue
            N = float(max(int(tv[k][i]), int(tv[k + 1][i])))

            def t_at(V_hist, A, C, B):
                return norm_t_batch(_rounding_hist(V_hist, A, C, B), dt)[:, i]

            # knob V: the base histogram changes
            lo, hi = sorted((_bits_of(vs[k]), _bits_of(vs[k + 1]))) if vs[k] * vs[k + 1] > 0 else (None, None)
            if lo is None:
                continue
            cache = {}

            def hist_v(b):
                if b not in cache:
                    cache[b] = base_hist(_float_of(b))
                return cache[b]

            try:
                vpair = _bisect(lambda b: t_at(hist_v(b), mid["A"], mid["C"], mid["B"])[0] >= N, lo, hi)
            except AssertionError:
                continue
            state = None
            for vb in vpair:                                   # whichever side the finer knobs can cross from
                st = dict(V=_float_of(vb), A=mid["A"], C=mid["C"], B=mid["B"])
                h = hist_v(vb)
                ok = True
                for knob in ("A", "B", "C"):
                    a, b = (_bits_of(x) for x in ROUND_RANGES[knob])

                    def pred(bits, knob=knob):
                        q = dict(st)
                        q[knob] = _float_of(bits)
                        return t_at(h, q["A"], q["C"], q["B"])[0] >= N
                    if pred(a) == pred(b):
                        ok = False
                        break
                    x0, x1 = _bisect(pred, a, b)
                    pair = (x0, x1)
                    st[knob] = _float_of(x0)
                if ok:
                    state = (st, h, pair)
                    break
            if state is None:
                continue
            st, h, pair = state
            # the last knob, a few hundred patterns around the crossing: keep one just below N and one at / above it
            cb = np.arange(pair[0] - 256, pair[1] + 257, dtype=np.int64).astype(np.uint32)
            tt = t_at(h, st["A"], cb.view(F), st["B"])
            u = np.spacing(N)
            below, above = np.nonzero((tt < N) & (N - tt <= u))[0], np.nonzero((tt >= N) & (tt - N <= u))[0]
            if not len(below) or not len(above):
                continue
            for side, q in (("below", below[len(below) // 2]), ("at_or_above", above[len(above) // 2])):
                out.append(_rec("norm/round_t%d_%d_%s" % (dt, found, side), "norm",
                                _rounding_patch(base, st["V"], st["A"], cb.view(F)[q], st["B"]), inexact={0: "small_term"},
                                rounding=dict(desc_type=dt, index=int(i), N=int(N), side=side)))
            found += 1
        assert found == NORM_SEARCH_COUNT, (dt, found)
    return out


def _random():
    rs = np.random.RandomState(4501)
    out = []
    for i in range(RANDOM_PER_KIND):
        kinds = (("smooth", OC._smooth(rs.standard_normal((PS, PS)).astype(F) * F(60), 1 + i % 4) + F(20)),
                 ("white", (rs.standard_normal((PS, PS)) * 40).astype(F)),
                 ("lowcontrast", OC._smooth((rs.standard_normal((PS, PS)) * (1.5 + 0.05 * i)).astype(F), 1) + F(100)),
                 ("integer", np.round(OC._smooth(rs.standard_normal((PS, PS)).astype(F) * F(90), 2) + F(128))))
        for kind, p in kinds:
            out.append(_rec("random/%s_%02d" % (kind, i), "random", p))
    for name, p in LC.cases():
        out.append(_rec("random/liop_" + name, "random", p))
    return out


def planted():
    """every planted patch, built once: list of dict(name, family, patch, options, claim)"""
    global _planted
    if _planted is None:
        _planted = _ramps() + _photometric() + _gather() + _magnitude() + _norm() + _random()
        assert len({c["name"] for c in _planted}) == len(_planted)
        for c in _planted:
            assert c["patch"].shape == (PS, PS) and c["patch"].dtype == F and np.isfinite(c["patch"]).all(), c["name"]
            c["patch"].setflags(write=False)
    return _planted


def by_name(name):
    return next(c for c in planted() if c["name"] == name)


def family_counts():
    out = {}
    for c in planted():
        out[c["family"]] = out.get(c["family"], 0) + 1
    return out


def raw_compared(case):
    """whether the raw histogram of the case is compared with dspsift_model.raw (16 ms a patch): every case but 7 in 8 of the
    plain table ramps"""
    n = case["name"]
    if not n.startswith("sift/ramp/c") or "rounded" in n:
        return True
    code, idx = case["claim"]["entry"]
    return (idx + code) % 8 == 0


# ---- the launch rule --------------------------------------------------------------------------------------------------------------
def launch_order(centres):
    """indices of a call's regions (one image, integer centres (x, y)) in k_describe's launch order"""
    c = np.asarray(centres, np.int64).reshape(-1, 2)
    key = (np.clip(c[:, 1] >> 6, 0, 1023) << 16) | np.clip(c[:, 0], 0, 65535)
    return np.argsort(key, kind="stable")


def workgroups(centres):
    """[(i, j)]: the call's regions in slots 0 and 1 of every workgroup (j == i for the last region of an odd call)"""
    o = launch_order(centres).tolist()
    return [(o[k], o[k + 1] if k + 1 < len(o) else o[k]) for k in range(0, len(o), 2)]


def predicted_ordered(centres, inexact):
    """ordered_workgroups the call adds: the workgroups with a region that needs the ordered gather"""
    return sum(1 for i, j in workgroups(centres) if inexact[i] or inexact[j])


# ---- images -----------------------------------------------------------------------------------------------------------------------
def compose(stack):
    """patches [n, 41, 41] -> list of dict(img f32, first, centres [m, 2] (x, y) of the cases first .. first + m - 1, left [m, 2],
    right [m, 2]: the blank cells next to them)"""
    stack = np.asarray(stack, F)
    out = []
    per = PER_ROW * ROWS_PER_IMAGE
    for first in range(0, len(stack), per):
        part = stack[first:first + per]
        rows = (len(part) + PER_ROW - 1) // PER_ROW
        img = np.zeros((PITCH_Y * rows, 2 * X0 + PITCH_X * 2 * PER_ROW + 1), F)
        k = np.arange(len(part))
        cx, cy = X0 + PITCH_X * (2 * (k % PER_ROW) + 1), Y0 + PITCH_Y * (k // PER_ROW)
        for q in range(len(part)):
            img[cy[q] - HALF:cy[q] + HALF + 1, cx[q] - HALF:cx[q] + HALF + 1] = part[q]
        out.append(dict(img=img, first=first, centres=np.stack([cx, cy], 1), left=np.stack([cx - PITCH_X, cy], 1),
                        right=np.stack([cx + PITCH_X, cy], 1)))
    return out


def compose_compact(stack):
    """(img, centres): every patch in a 42 x 42 cell of ONE image, no blank cells between them (the ramps as one call)"""
    stack = np.asarray(stack, F)
    n = len(stack)
    per_row = int(np.ceil(np.sqrt(n)))
    rows = (n + per_row - 1) // per_row
    img = np.zeros((2 * 4 + rows * PITCH_X, 2 * 4 + per_row * PITCH_X), F)
    k = np.arange(n)
    cx, cy = X0 + PITCH_X * (k % per_row), X0 + PITCH_X * (k // per_row)
    for q in range(n):
        img[cy[q] - HALF:cy[q] + HALF + 1, cx[q] - HALF:cx[q] + HALF + 1] = stack[q]
    return img, np.stack([cx, cy], 1)


_images = None


def image_params():
    """[(image index, photo_norm)] of every image of images() under every photo_norm of its families, from the constants alone"""
    out, k = [], 0
    for g, n in zip(GROUPS, IMAGES_PER_GROUP):
        for _ in range(n):
            out += [(k, pn) for pn in OPTIONS[g[0]]["photo_norm"]]
            k += 1
    return out


def images():
    """the image sets of GROUPS: list of dict(group, cases (indices into planted()), img, centres, left, right)"""
    global _images
    if _images is None:
        _images = []
        pl = planted()
        for g in GROUPS:
            idx = [i for i, c in enumerate(pl) if c["family"] in g]
            for im in compose(np.stack([pl[i]["patch"] for i in idx])):
                m = len(im["centres"])
                _images.append(dict(group="+".join(g), cases=idx[im["first"]:im["first"] + m], img=im["img"], centres=im["centres"],
                                    left=im["left"], right=im["right"], options=pl[idx[0]]["options"]))
    return _images


def regions(dtype, centres, s=1.0):
    c = np.asarray(centres, np.float64).reshape(-1, 2)
    one, zero = np.ones(len(c)), np.zeros(len(c))
    return OC.region_records(dtype, np.column_stack([c[:, 0], c[:, 1], s * one, one, zero, zero, one]))


# ---- references, computed once per process and shared ------------------------------------------------------------------------------
_ref = {}


def reference(oracle, i, photo_norm):
    """dict(patch: what the gather sees (the oracle's normalised patch), desc {0, 1}: oracle.describe_patch, decision:
    sift_gather_model.decide) of planted()[i]; `raw` and the Half descriptors (dspsift_model) are added by raw_of / desc_of"""
    key = (i, photo_norm)
    if key not in _ref:
        p = planted()[i]["patch"]
        d1, npatch = oracle.describe_patch(p, photo_norm=photo_norm, rootsift=1)
        d0, _ = oracle.describe_patch(p, photo_norm=photo_norm, rootsift=0)
        _ref[key] = dict(patch=npatch.reshape(PS, PS), desc={0: d0, 1: d1}, decision=G.decide(npatch))
    return _ref[key]


def hist_of(oracle, i, photo_norm):
    r = reference(oracle, i, photo_norm)
    if "hist" not in r:
        with np.errstate(all="ignore"):
            r["hist"] = D.histogram_f64(r["patch"])
    return r["hist"]


def raw_of(oracle, i, photo_norm):
    with np.errstate(all="ignore"):
        return hist_of(oracle, i, photo_norm).astype(F)


def desc_of(oracle, i, photo_norm, desc_type):
    """the reference descriptor: the oracle's for SIFT and RootSIFT, dspsift_model's f64 norms on its histogram for the Half types
    (the CPU test ties those norms to the oracle on every case for types 0 and 1)"""
    r = reference(oracle, i, photo_norm)
    if desc_type not in r["desc"]:
        r["desc"][desc_type] = D.describe_f64(hist_of(oracle, i, photo_norm), desc_type)
    return r["desc"][desc_type]


def inexact_of(oracle, i, photo_norm):
    return reference(oracle, i, photo_norm)["decision"]["inexact"]
