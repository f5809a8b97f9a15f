"""A numpy restatement of the reference's DAISY descriptor functor (DAISYDescriptor::operator(), descriptors/daisydescriptor.hpp
-> libdaisy: daisy.cpp, daisy.h, kutility/math.hpp, kutility/convolution_default.h) for the 41 x 41 patch that DescribeRegions<>
hands it.  The oracle of tests/test_gpu_daisy.py; checked bit for bit against the compiled reference through
tests/golden/daisy_ref.npz (tests/test_daisy_model_cpu.py, tools/make_daisy_fixture.py).

Every f32 operation is a numpy float32 operation, in the reference's order; the patches of a call are elements of the arrays, so
each patch sees the scalar chain of the reference:
  1. bytes: rint (half to even) and saturation to 0 .. 255, then f32 * (float)(1.0 / 255.0);
  2. a 5-tap gaussian (sigma 0.5) over all rows, then over all columns, borders replicated; each output is the chain sum = 0;
     sum += in[i + j] * k[j] for j = 0 .. ksize - 1; central differences halved (in double: exact), one-sided at the borders;
     layer l = max(kos_l * dx + zin_l * dy, 0), kos / zin the f32 of the double cos / sin of the f32 angle 2 l pi / 8;
  3. every layer smoothed with sigma (float)sqrt(1.6^2 - 0.25);
  4. cube r from cube r - 1 with sigma sqrt(s_r^2 - s_{r-1}^2), s_r = (r + 1) (rad / radq) / 2;
  5. the centre and radq x thq grid points, each a bilinear mix w0 A + w1 C + w2 B + w3 D of its ring's cube, skipped (left 0)
     outside [0, 40), zeroed where int(x) or int(y) >= 39;
  6. NRM_PARTIAL (each histogram by its norm unless that is 0), NRM_FULL, or NRM_SIFT (up to 5 rounds of: divide by the norm when
     it exceeds 1e-5, clip at 0.154f; stop after a round that clipped nothing).
The gaussian taps call the f32 exponential of the C library and cos / sin the double ones (the reference's object imports expf
and sincos).  variant = "swap" (columns before rows) or "reverse" (taps in reverse order) are wrong on purpose: the tests use them
to show that the cases pin the order."""
import ctypes
import ctypes.util
import functools
import math

import numpy as np

F = np.float32
L = 41
NPX = L * L
HISTQ = 8
MAX_DIM = 200
MAX_TAPS = 51
SKIPPED, ZEROED, SAMPLED = 0, 1, 2
NRM_PARTIAL, NRM_FULL, NRM_SIFT = 0, 1, 2
CLIP = F(0.154)
MAX_ROUNDS = 5
PI = 3.141592653589793                      # kutility_def.hpp
PI_F = F(math.atan2(0.0, -1.0))             # kutility::pi(): atan2 of two floats, returned as float

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def expf(x):
    return F(_libm.expf(ctypes.c_float(float(F(x)))))


def dim(radq, thq, histq=HISTQ):
    return (radq * thq + 1) * histq


def filter_size(sigma):
    """daisy::filter_size(double)"""
    fsz = int(5 * float(sigma))
    if fsz % 2 == 0:
        fsz += 1
    return max(fsz, 3)


def gaussian_1d(fsz, sigma):
    """kutility::gaussian_1d(fltr, fsz, (float)sigma, 0.0f)"""
    sigma = F(sigma)
    sz = (fsz - 1) // 2
    v = F(F(F(2) * sigma) * sigma)
    out = np.zeros(fsz, F)
    s = F(0)
    for i, x in enumerate(range(-sz, sz + 1)):
        d = F(F(x) - F(0))
        out[i] = expf(F(F(-d) * d) / v)
        s = F(s + out[i])
    if s != 0:
        for i in range(fsz):
            out[i] = F(out[i] / s)
    return out


@functools.lru_cache(maxsize=None)
def tables(rad=15, radq=3, thq=8, histq=HISTQ):
    """dict(k5 [5], kos [8], zin [8], fsz [1 + radq], taps [1 + radq][51] (zero beyond fsz), sigmas [1 + radq] f64, selected
    [radq], cube / state / base [npts], w [npts][4], grid [npts][2] f64 (y, x offsets)); filter 0 is the smoothing of the layers,
    filter 1 + r makes cube r"""
    assert histq == HISTQ
    npts = radq * thq + 1
    radf = F(rad)
    kos, zin = np.zeros(8, F), np.zeros(8, F)
    for l in range(histq):
        angle = F(F(F(2 * l) * PI_F) / F(histq))
        kos[l], zin[l] = F(math.cos(float(angle))), F(math.sin(float(angle)))
    cs = [(r + 1) * (float(radf) / radq) / 2 for r in range(radq)]
    sig = [float(F(math.sqrt(1.6 * 1.6 - 0.25)))]
    for r in range(radq):
        sig.append(cs[0] if r == 0 else math.sqrt(cs[r] * cs[r] - cs[r - 1] * cs[r - 1]))
    fsz = np.array([filter_size(s) for s in sig], np.int32)
    taps = np.zeros((1 + radq, MAX_TAPS), F)
    for i, s in enumerate(sig):
        taps[i, :fsz[i]] = gaussian_1d(int(fsz[i]), s)
    # update_selected_cubes / quantize_radius(float)
    selected = np.zeros(radq, np.int32)
    for r in range(radq):
        seed = float(F(F(F(r + 1) * radf) / F(radq))) / 2.0
        q = float(F(seed))
        if q <= cs[0]:
            selected[r] = 0
        elif q >= cs[-1]:
            selected[r] = radq - 1
        else:
            best = np.finfo(F).max
            for c in range(radq):
                d = F(abs(cs[c] - q))
                if d < best:
                    best, selected[r] = d, c
    # compute_grid_points (r_step is an f32 quotient), compute_oriented_grid_points at orientation 0
    r_step = float(F(radf / F(radq)))
    t_step = 2 * PI / thq
    grid = np.zeros((npts, 2), np.float64)
    kz, zz = math.cos(-0.0), math.sin(-0.0)
    for r in range(radq):
        for t in range(thq):
            x = ((r + 1) * r_step) * math.cos(t * t_step)
            y = ((r + 1) * r_step) * math.sin(t * t_step)
            grid[1 + r * thq + t] = (-x * zz + y * kz, x * kz + y * zz)
    cube = np.zeros(npts, np.int32)
    state, base, w = np.zeros(npts, np.int32), np.zeros(npts, np.int32), np.zeros((npts, 4), F)
    c0 = float(L // 2)
    for g in range(npts):
        cube[g] = selected[0] if g == 0 else selected[(g - 1) // thq]
        yy, xx = c0 + grid[g, 0], c0 + grid[g, 1]
        if g > 0 and not (0 <= xx < L - 1 and 0 <= yy < L - 1):
            state[g] = SKIPPED
            continue
        mnx, mny = int(xx), int(yy)
        if mnx >= L - 2 or mny >= L - 2:
            state[g] = ZEROED
            continue
        alpha, beta = mnx + 1 - xx, mny + 1 - yy
        w0 = F(alpha * beta)
        state[g], base[g] = SAMPLED, mny * L + mnx
        w[g] = (w0, F(beta - float(w0)), F(alpha - float(w0)), F(float(F(F(1) + w0)) - alpha - beta))
    out = dict(k5=gaussian_1d(5, 0.5), kos=kos, zin=zin, fsz=fsz, taps=taps, sigmas=np.array(sig), selected=selected, cube=cube,
               state=state, base=base, w=w, grid=grid)
    for v in out.values():
        v.setflags(write=False)
    return out


def to_unit(patches):
    """step 1: [..][41][41] f32 -> bytes as f32 * (float)(1.0 / 255.0)"""
    b = np.clip(np.rint(np.asarray(patches, F)), F(0), F(255)).astype(F)
    return b * F(1.0 / 255.0)


def conv_axis(a, k, axis, reverse=False):
    """conv_horizontal (axis -1) / conv_vertical (axis -2): replicated borders, the ordered chain of conv_buffer_"""
    k = np.asarray(k, F)
    half = len(k) // 2
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (half, half)
    p = np.pad(a, pad, mode="edge")
    s = np.zeros_like(a)
    order = range(len(k) - 1, -1, -1) if reverse else range(len(k))
    for j in order:
        s = s + np.take(p, range(j, j + n), axis=axis) * k[j]
    return s


def convolve_sym(a, k, variant=None):
    if variant == "swap":
        return conv_axis(conv_axis(a, k, -2), k, -1)
    return conv_axis(conv_axis(a, k, -1, variant == "reverse"), k, -2, variant == "reverse")


def gradient(im):
    """kutility::gradient -> dx, dy"""
    dx, dy = np.zeros_like(im), np.zeros_like(im)
    dx[..., 1:-1] = ((im[..., 2:] - im[..., :-2]).astype(np.float64) / 2.0).astype(F)
    dx[..., 0] = im[..., 1] - im[..., 0]
    dx[..., -1] = im[..., -1] - im[..., -2]
    dy[..., 1:-1, :] = ((im[..., 2:, :] - im[..., :-2, :]).astype(np.float64) / 2.0).astype(F)
    dy[..., 0, :] = im[..., 1, :] - im[..., 0, :]
    dy[..., -1, :] = im[..., -1, :] - im[..., -2, :]
    return dx, dy


def l2norm(a):
    """kutility::l2norm over the last axis: an ordered f32 sum of squares, then the f32 root"""
    s = np.zeros(a.shape[:-1], F)
    for k in range(a.shape[-1]):
        s = s + a[..., k] * a[..., k]
    return np.sqrt(s)


def _inv(norm):
    with np.errstate(divide="ignore"):
        return (1.0 / norm.astype(np.float64)).astype(F)


def normalize(desc, nrm_type, histq=HISTQ, info=None):
    """step 6 on [n][dim] f32 (a copy is returned)"""
    d = np.array(desc, F)
    n = len(d)
    if nrm_type == NRM_PARTIAL:
        h = d.reshape(n, d.shape[1] // histq, histq)
        norm = l2norm(h)
        nz = norm != 0
        h[nz] = h[nz] * _inv(norm)[nz][:, None]
        if info is not None:
            info["zero_hist"] = ~nz
    elif nrm_type == NRM_FULL:
        norm = l2norm(d)
        nz = norm != 0
        d[nz] = d[nz] * _inv(norm)[nz][:, None]
        if info is not None:
            info["zero_norm"] = ~nz
    elif nrm_type == NRM_SIFT:
        changed = np.ones(n, bool)
        rounds, clips = np.zeros(n, np.int32), np.zeros((n, MAX_ROUNDS), np.int32)
        for it in range(MAX_ROUNDS):
            act = changed.copy()
            if not act.any():
                break
            norm = l2norm(d)
            div = act & (norm.astype(np.float64) > 1e-5)
            d[div] = d[div] * _inv(norm)[div][:, None]
            clip = act[:, None] & (d > CLIP)
            d[clip] = CLIP
            changed = clip.any(1)
            rounds += act
            clips[:, it] = clip.sum(1)
        if info is not None:
            info["rounds"], info["clips"] = rounds, clips
    else:
        raise ValueError(nrm_type)
    return d


def describe(patches, rad=15, radq=3, thq=8, histq=HISTQ, nrm_type=NRM_PARTIAL, info=None, variant=None):
    """[n][41][41] f32 -> [n][(radq * thq + 1) * 8] f32.  info (a dict) receives blurred, dx, dy [n][41][41], cubes
    [radq][n][8][41][41], raw [n][dim] (before step 6) and what normalize() reports"""
    T = tables(rad, radq, thq, histq)
    p = np.asarray(patches, F).reshape(-1, L, L)
    n = len(p)
    im = convolve_sym(to_unit(p), T["k5"], variant)
    dx, dy = gradient(im)
    v = T["kos"][None, :, None, None] * dx[:, None] + T["zin"][None, :, None, None] * dy[:, None]
    cur = np.where(v > 0, v, F(0)).astype(F)
    cur = convolve_sym(cur, T["taps"][0, :T["fsz"][0]], variant)
    cubes = []
    for r in range(radq):
        cur = convolve_sym(cur, T["taps"][1 + r, :T["fsz"][1 + r]], variant)
        cubes.append(cur)
    npts = radq * thq + 1
    raw = np.zeros((n, npts, histq), F)
    for g in range(npts):
        if T["state"][g] != SAMPLED:
            continue
        c = cubes[T["cube"][g]].reshape(n, histq, NPX)
        b, w = int(T["base"][g]), T["w"][g]
        h = w[0] * c[:, :, b]
        h = h + w[1] * c[:, :, b + 1]
        h = h + w[2] * c[:, :, b + L]
        h = h + w[3] * c[:, :, b + L + 1]
        raw[:, g] = h
    raw = raw.reshape(n, npts * histq)
    if info is not None:
        info.update(blurred=im, dx=dx, dy=dy, cubes=np.stack(cubes), raw=raw)
    return normalize(raw, nrm_type, histq, info)
