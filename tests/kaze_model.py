"""A numpy restatement of the KAZE detector the library runs on the GPU: the reference's "KAZE" branch
(imagerepresentation.cpp:678-681, 1132-1152), which runs aka::AKAZE::Create_Nonlinear_Scale_Space and Feature_Detection
(akaze/src/lib/AKAZE.cpp, nldiffusion_functions.cpp, fed.cpp) on the view / 255, with every f32 operation in the reference's order
and the OpenCV calls as tools/kaze_standin/opencv2/opencv.hpp specifies them (include/modsx.h restates the rules):
  levels / fed_tau   Allocate_Memory_Evolution and fed_tau_by_process_time with reordering;
  blur               GaussianBlur(BORDER_REPLICATE) by the project's gaussian_kernel and pass order, with AKAZE's size rule;
  sep3               the three non-zero taps of a Scharr or compute_derivative_kernels pass at distance s, BORDER_REFLECT_101;
  k_percentile       compute_k_percentile, the float counters as min(count, 2^24);
  pm_g2, nld_step    the conductivity and one explicit diffusion step with its four one-sided border strips;
  halfsample         resize(INTER_AREA): the exact 2 x 2 mean or the area table;
  ldet               Compute_Multiscale_Derivatives and the determinant, without FMA;
  find / refine      Find_Scale_Space_Extrema (raw maxima, the same-level / lower-level pass, the upper-level pass) and
                     Do_Subpixel_Refinement with the 2 x 2 solve.
detect() reports every stage and counters of what the case exercised."""
import ctypes
import ctypes.util
import hashlib
import math

import numpy as np

F = np.float32
D = np.float64
DET_KAZE = 9
DEFAULTS = dict(omax=4, nsublevels=4, soffset=1.6, derivative_factor=1.5, dthreshold=0.001, min_dthreshold=1e-5,
                kcontrast_percentile=0.7, kcontrast_nbins=300, descriptor=5)
MAX_S = 8           # the largest derivative distance the library's tiles hold

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def powf(a, b):
    return F(_libm.powf(float(F(a)), float(F(b))))


def fround(v):
    """aka::fRound: (int)(flt + 0.5f), truncation toward zero"""
    return int(np.trunc(F(v) + F(0.5)))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def smax_of(descriptor):
    if descriptor in (0, 1, 4, 5):
        return F(10.0 * float(np.sqrt(F(2.0))))
    if descriptor in (2, 3):
        return F(12.0 * float(np.sqrt(F(2.0))))
    return F(0.0)


def is_prime(n):
    if n <= 1:
        return False
    if n in (2, 3, 5, 7):
        return True
    if n % 2 == 0 or n % 3 == 0 or n % 5 == 0 or n % 7 == 0:
        return False
    prime, upper, d = True, int(math.sqrt(n + 1.0)), 11
    while d <= upper:
        if n % d == 0:
            prime = False
        d += 2
    return prime


def fed_tau(T, tau_max=0.25, reordering=True):
    """fed_tau_by_process_time(T, 1, tau_max, reordering) -> f32 list"""
    t, tau_max = F(F(T) / F(1)), F(tau_max)
    n = int(math.ceil(math.sqrt(3.0 * float(t) / float(tau_max) + 0.25) - 0.5 - float(F(1.0e-8))) + 0.5)
    if n <= 0:
        return np.zeros(0, F)
    scale = F(3.0 * float(t) / float(tau_max * F(n * (n + 1))))
    c = F(1.0) / (F(4.0) * F(n) + F(2.0))
    d = scale * tau_max / F(2.0)
    tauh = np.zeros(n, F)
    for k in range(n):
        h = F(math.cos(math.pi * float(F(2.0) * F(k) + F(1.0)) * float(c)))
        tauh[k] = d / (h * h)
    if not reordering:
        return tauh
    kappa, prime = n // 2, n + 1
    while not is_prime(prime):
        prime += 1
    tau, k = np.zeros(n, F), 0
    for l in range(n):
        while True:
            index = ((k + 1) * kappa) % prime - 1
            if index < n:
                break
            k += 1
        tau[l] = tauh[index]
        k += 1
    return tau


def levels(rows, cols, reordering=True, **kw):
    """-> (list of dict(octave, sublevel, rows, cols, esigma, etime, sigma_size, dsize (the derivative distance), ksize, tau), omax)"""
    p = params(**kw)
    out, omax = [], p["omax"]
    for i in range(p["omax"]):
        rfactor = F(1.0 / float(powf(2.0, i)))
        h, w = int(F(rows) * rfactor), int(F(cols) * rfactor)
        if (w < 80 or h < 40) and i != 0:
            omax = i
            break
        for j in range(p["nsublevels"]):
            esigma = F(p["soffset"]) * powf(2.0, F(j) / F(p["nsublevels"]) + F(i))
            ratio = powf(2.0, F(i))
            dsize = fround(esigma * F(p["derivative_factor"]) / ratio)
            out.append(dict(octave=i, sublevel=j, rows=h, cols=w, esigma=esigma, etime=F(0.5 * float(esigma * esigma)),
                            sigma_size=fround(esigma), dsize=dsize, ksize=3 + 2 * (dsize - 1), tau=np.zeros(0, F)))
    for i in range(1, len(out)):
        out[i]["tau"] = fed_tau(out[i]["etime"] - out[i - 1]["etime"], reordering=reordering)
    return out, omax


def gaussian_kernel(n, sigma):
    sigma = float(sigma) if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    s2 = -0.5 / (sigma * sigma)
    k = np.array([math.exp(s2 * (i - (n - 1) * 0.5) * (i - (n - 1) * 0.5)) for i in range(n)]).astype(F)
    tot = 0.0
    for v in k:
        tot += float(v)
    return (k.astype(D) * (1.0 / tot)).astype(F)


def blur_ksize(sigma):
    """gaussian_2D_convolution's size rule: ceil(2 (1 + (sigma - 0.8) / 0.3)) made odd"""
    n = int(math.ceil(2.0 * (1.0 + (float(F(sigma)) - 0.8) / 0.3)))
    return n + 1 if n % 2 == 0 else n


def _idx(n, k, border):
    i = np.arange(n) + k
    if border == "replicate":
        return np.clip(i, 0, n - 1)
    if n == 1:
        return np.zeros(n, int)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)
    return i


def blur(img, n, sigma, border="replicate"):
    """the project's two-pass Gaussian (oracle.gaussian_blur_xy's order) with an n-tap kernel"""
    img = np.asarray(img, F)
    rows, cols = img.shape
    nx, ny = (1 if cols == 1 else n), (1 if rows == 1 else n)
    KX, KY = gaussian_kernel(nx, sigma), gaussian_kernel(ny, sigma)
    rx, ry = nx // 2, ny // 2
    if nx <= 5:
        t = img * KX[rx]
        for j in range(1, rx + 1):
            t = t + (img[:, _idx(cols, -j, border)] + img[:, _idx(cols, j, border)]) * KX[rx + j]
    else:
        t = np.zeros_like(img)
        for j in range(nx):
            t = t + img[:, _idx(cols, j - rx, border)] * KX[j]
    o = KY[ry] * t + F(0.0)
    for j in range(1, ry + 1):
        o = o + KY[ry + j] * (t[_idx(rows, j, border)] + t[_idx(rows, -j, border)])
    assert o.dtype == F
    return o


def sep3(a, axis, taps, s, order="ascending"):
    """one pass of sepFilter2D with the three non-zero taps (k0, k1, k2) at -s, 0, +s along axis, BORDER_REFLECT_101; taps in
    ascending index order, every product and add rounded, from the first product.  k1 None: the tap is 0 and is skipped (it adds
    +-0).  order "descending" is the deliberate mistake of tests/test_kaze_model_cpu.py."""
    n = a.shape[axis]
    lo, hi = np.take(a, _idx(n, -s, "reflect"), axis=axis), np.take(a, _idx(n, s, "reflect"), axis=axis)
    k0, k1, k2 = (F(t) if t is not None else None for t in taps)
    if order != "ascending":
        lo, hi, k0, k2 = hi, lo, k2, k0
    v = lo * k0
    if k1 is not None:
        v = v + a * k1
    v = v + hi * k2
    assert v.dtype == F
    return v


DERIV = (-1.0, None, 1.0)


def smooth_taps(s):
    """compute_derivative_kernels' order-0 kernel of scale s (s = 1: getDerivKernels normalised, [3, 10, 3] / 32)"""
    if s == 1:
        return (F(3.0 / 32), F(10.0 / 32), F(3.0 / 32))
    w = F(10.0 / 3.0)
    norm = F(1.0 / (2.0 * s * (float(w) + 2.0)))
    return (norm, w * norm, norm)


def first_derivs(a, s, taps, order="ascending"):
    """Lx = columns(smooth) of rows(deriv), Ly = columns(deriv) of rows(smooth)"""
    return (sep3(sep3(a, 1, DERIV, s, order), 0, taps, s, order), sep3(sep3(a, 1, taps, s, order), 0, DERIV, s, order))


def scharr(a, order="ascending"):
    return first_derivs(a, 1, (3.0, 10.0, 3.0), order)


def k_percentile(img, perc, nbins):
    """compute_k_percentile(img, perc, 1.0, nbins, 0, 0) -> (k, hmax, hist int64, branch)"""
    g = blur(img, blur_ksize(1.0), 1.0)
    lx, ly = scharr(g)
    lx, ly = lx[1:-1, 1:-1], ly[1:-1, 1:-1]
    modg = np.sqrt(lx * lx + ly * ly)
    assert modg.dtype == F
    hmax = F(0.0)
    if modg.size:
        m = modg.max()
        hmax = m if m > hmax else hmax
    nz = modg[modg != 0]
    hist = np.zeros(nbins, np.int64)
    if nz.size:
        with np.errstate(all="ignore"):
            b = np.floor(F(nbins) * (nz / hmax)).astype(np.int64)
        b[b == nbins] = nbins - 1
        hist = np.bincount(b, minlength=nbins).astype(np.int64)
    cap = 1 << 24
    npoints = F(min(int(nz.size), cap))
    nthreshold = int(npoints * F(perc))
    nelements, k = 0, 0
    while nelements < nthreshold and k < nbins:
        nelements = int(F(nelements) + F(min(int(hist[k]), cap)))
        k += 1
    if nelements < nthreshold:
        return F(0.03), hmax, hist, "0.03"
    return hmax * (F(k) / F(nbins)), hmax, hist, "walk"


def pm_g2(lx, ly, k):
    with np.errstate(all="ignore"):
        inv = F(D(1.0) / D(F(k) * F(k)))
        return F(1.0) / (F(1.0) + (lx * lx + ly * ly) * inv)


def nld_step(L, c, tau):
    """nld_step_scalar: the new Lt.  0.5 * stepsize * (f32 sum) is an f64 product rounded on store; corners keep Lstep = 0"""
    rows, cols = L.shape
    step = np.zeros_like(L)
    with np.errstate(all="ignore"):
        def xp(r, j):
            return (c[r, j] + c[r, j + 1]) * (L[r, j + 1] - L[r, j])

        def xn(r, j):
            return (c[r, j - 1] + c[r, j]) * (L[r, j] - L[r, j - 1])

        def yp(r, j):
            return (c[r, j] + c[r + 1, j]) * (L[r + 1, j] - L[r, j])

        def yn(r, j):
            return (c[r - 1, j] + c[r, j]) * (L[r, j] - L[r - 1, j])

        def same(r, j):
            return (c[r, j] + c[r, j]) * (L[r, j] - L[r, j])
        half = 0.5 * float(F(tau))
        store = lambda s: (half * s.astype(D)).astype(F)                  # noqa: E731
        R, J = np.arange(1, rows - 1)[:, None], np.arange(1, cols - 1)[None, :]
        step[1:-1, 1:-1] = store(xp(R, J) - xn(R, J) + yp(R, J) - yn(R, J))
        j, r = np.arange(1, cols - 1), np.arange(1, rows - 1)
        step[0, 1:-1] = store(xp(0, j) - xn(0, j) + yp(0, j))
        step[-1, 1:-1] = store(xp(rows - 1, j) - xn(rows - 1, j) + same(rows - 1, j) - yn(rows - 1, j))
        step[1:-1, 0] = store(xp(r, 0) - same(r, 0) + yp(r, 0) - yn(r, 0))
        step[1:-1, -1] = store(-xn(r, cols - 1) + yp(r, cols - 1) - yn(r, cols - 1))
        out = L + step
    assert out.dtype == F
    return out


def area_table(ssize, dsize):
    scale = ssize / float(dsize)
    tab = []
    for d in range(dsize):
        fs1 = d * scale
        fs2 = fs1 + scale
        cell = min(scale, ssize - fs1)
        s2 = min(int(math.floor(fs2)), ssize - 1)
        s1 = min(int(math.ceil(fs1)), s2)
        e = []
        if s1 - fs1 > 1e-3:
            e.append((s1 - 1, F((s1 - fs1) / cell)))
        for s in range(s1, s2):
            e.append((s, F(1.0 / cell)))
        if fs2 - s2 > 1e-3:
            e.append((s2, F(min(min(fs2 - s2, 1.0), cell) / cell)))
        tab.append(e)
    return tab


def halfsample(a):
    """resize(src, dst(rows / 2, cols / 2), INTER_AREA) -> (dst, "exact" or "area")"""
    sr, sc = a.shape
    dr, dc = sr // 2, sc // 2
    if sr == 2 * dr and sc == 2 * dc:
        return (((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2]) + a[1::2, 1::2]) * F(0.25), "exact"
    xt, yt = area_table(sc, dc), area_table(sr, dr)
    nx = max(len(e) for e in xt)
    out = np.zeros((dr, dc), F)
    for r in range(dr):
        for k, (sy, beta) in enumerate(yt[r]):
            S = a[sy]
            buf = np.zeros(dc, F)
            for j in range(nx):
                has = np.array([len(e) > j for e in xt])
                si = np.array([e[j][0] if len(e) > j else 0 for e in xt])
                al = np.array([e[j][1] if len(e) > j else 0 for e in xt], F)
                buf = np.where(has, buf + S[si] * al, buf)
            out[r] = beta * buf if k == 0 else out[r] + beta * buf
    assert out.dtype == F
    return out, "area"


def ldet(lsmooth, s, order="ascending"):
    taps = smooth_taps(s)
    lx, ly = first_derivs(lsmooth, s, taps, order)
    lxx = sep3(sep3(lx, 1, DERIV, s, order), 0, taps, s, order)
    lyy = sep3(sep3(ly, 1, taps, s, order), 0, DERIV, s, order)
    lxy = sep3(sep3(lx, 1, taps, s, order), 0, DERIV, s, order)
    with np.errstate(all="ignore"):
        ss = F(s * s)
        lxx, lyy, lxy = lxx * ss, lyy * ss, lxy * ss
        out = lxx * lyy - lxy * lxy
    assert out.dtype == F
    return out


KP = np.dtype([("x", F), ("y", F), ("size", F), ("response", F), ("octave", np.int32), ("class_id", np.int32)])


def raw_maxima(planes, dthreshold, min_dthreshold):
    """the 3 x 3 scan in (level, raster) order -> [n][3] int32 (level, row, col), values f32"""
    pos, val = [], []
    for i, L in enumerate(planes):
        if L.shape[0] < 3 or L.shape[1] < 3:
            continue
        v = L[1:-1, 1:-1]
        with np.errstate(all="ignore"):
            keep = (v > F(dthreshold)) & (v >= F(min_dthreshold))
            for dr in (0, 1, 2):
                for dc in (0, 1, 2):
                    if dr != 1 or dc != 1:
                        keep &= v > L[dr:L.shape[0] - 2 + dr, dc:L.shape[1] - 2 + dc]
        r, c = np.nonzero(keep)
        pos.append(np.stack([np.full(len(r), i), r + 1, c + 1], axis=1).astype(np.int32))
        val.append(v[r, c])
    if not pos:
        return np.zeros((0, 3), np.int32), np.zeros(0, F)
    return np.concatenate(pos), np.concatenate(val).astype(F)


def find(raw, rawv, lv, shapes, **kw):
    """the two filter passes of Find_Scale_Space_Extrema over the raw maxima -> (aux, upper, stats)"""
    p = params(**kw)
    smax = smax_of(p["descriptor"])
    n = len(raw)
    a = np.zeros(n, KP)
    cnt = 0
    st = dict(same_keep=0, same_drop=0, lower_keep=0, lower_drop=0, replaced=0, upper_rejected=0, out_left=0, out_right=0, out_top=0,
              out_bottom=0, inside=np.zeros(len(lv), np.int64), maxima=np.bincount(raw[:, 0], minlength=len(lv)) if n else np.zeros(len(lv), np.int64))
    for (i, r, c), v in zip(raw, rawv):
        L = lv[i]
        size = L["esigma"] * F(p["derivative_factor"])
        ratio = F(2.0 ** L["octave"])
        ss = fround(size / ratio)
        x, y, resp = F(c), F(r), np.abs(v)
        keep, rep = True, -1
        if cnt:
            cl = a["class_id"][:cnt]
            dx, dy = (x * ratio - a["x"][:cnt]).astype(D), (y * ratio - a["y"][:cnt]).astype(D)
            dist = np.sqrt(dx * dx + dy * dy).astype(F)
            hit = np.nonzero(((cl == i) | (cl == i - 1)) & (dist <= size))[0]
            if len(hit):
                k = hit[0]
                kind = "same" if cl[k] == i else "lower"
                if resp > a["response"][k]:
                    rep = k
                    st[kind + "_keep"] += 1
                else:
                    keep = False
                    st[kind + "_drop"] += 1
        if not keep:
            continue
        m = smax * F(ss)
        lx, rx, uy, dy_ = fround(x - m) - 1, fround(x + m) + 1, fround(y - m) - 1, fround(y + m) + 1
        rows, cols = shapes[i]
        if lx < 0 or rx >= cols or uy < 0 or dy_ >= rows:
            st["out_left"] += lx < 0; st["out_right"] += rx >= cols; st["out_top"] += uy < 0; st["out_bottom"] += dy_ >= rows
            continue
        st["inside"][i] += 1
        rec = (x * ratio, y * ratio, size, resp, L["octave"], i)
        if rep < 0:
            a[cnt] = rec
            cnt += 1
        else:
            a[rep] = rec
            st["replaced"] += 1
    a = a[:cnt].copy()
    keep = np.ones(cnt, bool)
    for i in range(cnt):
        j = np.arange(i + 1, cnt)
        up = j[a["class_id"][j] == a["class_id"][i] + 1]
        if len(up):
            dx, dy = (a["x"][i] - a["x"][up]).astype(D), (a["y"][i] - a["y"][up]).astype(D)
            dist = np.sqrt(dx * dx + dy * dy).astype(F)
            if ((dist <= a["size"][i]) & (a["response"][i] < a["response"][up])).any():
                keep[i] = False
                st["upper_rejected"] += 1
    return a, a[keep].copy(), st


def solve2(A, b, dst):
    """cv::solve 2 x 2 DECOMP_LU as the stand-in specifies it; dst (f32 [2]) is left alone where the determinant is 0"""
    a00, a01, a10, a11 = (float(v) for v in A)
    b0, b1 = float(b[0]), float(b[1])
    d = a00 * a11 - a01 * a10
    if d != 0.0:
        d = 1.0 / d
        dst[0], dst[1] = F((b0 * a11 - b1 * a01) * d), F((b1 * a00 - b0 * a10) * d)
        return True
    return False


def refine(kps, planes, lv):
    """Do_Subpixel_Refinement -> (final, stats)"""
    out = []
    dst = np.zeros(2, F)
    st = dict(erased=0, singular_first=0, singular_after=0, solved=0)
    with np.errstate(all="ignore"):
        for k in kps:
            ratio = F(2.0 ** int(k["octave"]))
            x, y = fround(k["x"] / ratio), fround(k["y"] / ratio)
            L = planes[int(k["class_id"])]
            at = lambda r, c: L[r, c]                                   # noqa: E731
            Dx = F(0.5 * float(at(y, x + 1) - at(y, x - 1)))
            Dy = F(0.5 * float(at(y + 1, x) - at(y - 1, x)))
            Dxx = F(float(at(y, x + 1) + at(y, x - 1)) - 2.0 * float(at(y, x)))
            Dyy = F(float(at(y + 1, x) + at(y - 1, x)) - 2.0 * float(at(y, x)))
            Dxy = F(0.25 * float(at(y + 1, x + 1) + at(y - 1, x - 1)) - 0.25 * float(at(y - 1, x + 1) + at(y + 1, x - 1)))
            if solve2((Dxx, Dxy, Dxy, Dyy), (-Dx, -Dy), dst):
                st["solved"] += 1
            else:
                st["singular_after" if st["solved"] else "singular_first"] += 1
            if np.abs(dst[0]) <= 1.0 and np.abs(dst[1]) <= 1.0:
                up = F(2.0 ** lv[int(k["class_id"])]["octave"])
                r = k.copy()
                r["x"], r["y"] = (F(x) + dst[0]) * up, (F(y) + dst[1]) * up
                r["size"] = F(float(k["size"]) * 2.0)
                out.append(r)
            else:
                st["erased"] += 1
    return (np.array(out, KP) if out else np.zeros(0, KP)), st


def scan(planes, lv, **kw):
    """the extrema scan, both filter passes and the refinement on given Ldet planes (modsx_debug_kaze_scan)"""
    p = params(**kw)
    raw, rawv = raw_maxima(planes, p["dthreshold"], p["min_dthreshold"])
    aux, upper, st = find(raw, rawv, lv, [a.shape for a in planes], **kw)
    final, st2 = refine(upper, planes, lv)
    st.update(st2)
    return dict(raw=raw, rawv=rawv, aux=aux, upper=upper, final=final, stats=st)


def detect(img, tap_order="ascending", reordering=True, **kw):
    """-> dict(levels, omax, kcontrast, hmax, hist, Lt, Lsmooth, Lflow, Ldet (lists of planes), raw, rawv, aux, upper, final, stats)"""
    p = params(**kw)
    img = np.asarray(img, F)
    lv, omax = levels(img.shape[0], img.shape[1], reordering=reordering, **kw)
    g = img * F(1.0 / 255.0)
    k, hmax, hist, branch = k_percentile(g, p["kcontrast_percentile"], p["kcontrast_nbins"])
    Lt = [blur(g, blur_ksize(p["soffset"]), float(F(p["soffset"])))]
    Lsmooth, Lflow = [Lt[0]], [np.zeros_like(g)]
    resize = set()
    kc = k
    for i in range(1, len(lv)):
        if lv[i]["octave"] > lv[i - 1]["octave"]:
            cur, how = halfsample(Lt[i - 1])
            resize.add(how)
            kc = F(float(kc) * 0.75)
        else:
            cur = Lt[i - 1]
        sm = blur(cur, blur_ksize(1.0), 1.0)
        lx, ly = scharr(sm, tap_order)
        flow = pm_g2(lx, ly, kc)
        for tau in lv[i]["tau"]:
            cur = nld_step(cur, flow, tau)
        Lt.append(cur); Lsmooth.append(sm); Lflow.append(flow)
    Ldet = [ldet(Lsmooth[i], lv[i]["dsize"], tap_order) for i in range(len(lv))]
    out = scan(Ldet, lv, **kw)
    out["stats"].update(k_branch=branch, resize=sorted(resize))
    out.update(levels=lv, omax=omax, kcontrast=k, hmax=hmax, hist=hist, Lt=Lt, Lsmooth=Lsmooth, Lflow=Lflow, Ldet=Ldet)
    return out


def keypoints(final, dtype):
    """the det_kp of the reference's KAZE branch (imagerepresentation.cpp:1140-1151): widened f32, orientation 0"""
    k = np.zeros(len(final), dtype)
    k["x"], k["y"], k["response"] = final["x"].astype(D), final["y"].astype(D), final["response"].astype(D)
    k["s"] = final["size"].astype(D) / 3.0
    k["a11"], k["a12"], k["a21"], k["a22"] = np.cos(0.0), np.sin(0.0), -np.sin(0.0), np.cos(0.0)
    k["octave_number"] = final["octave"]
    return k


def digest(a):
    """SHA-256 of a plane's bytes with -0 stored as +0 and every NaN as the one quiet NaN (nothing downstream tells them apart)"""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        with np.errstate(all="ignore"):
            a = np.where(np.isnan(a), a.dtype.type(np.nan), a + a.dtype.type(0))
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def sample_index(n, seed=9173, k=64):
    """the k seeded flat indices at which the fixture samples a plane of n values"""
    return np.random.default_rng(seed + n).integers(0, n, k)


def same(a, b):
    """equality of f32 planes in which -0 and +0 compare equal and NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
