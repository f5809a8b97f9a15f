"""A numpy restatement of the SURF detector the library runs on the GPU (OpenSURF's FastHessian: opensurf/integral.cpp,
integral.h, responselayer.h, fasthessian.cpp), with every f32 operation in the reference's order:
  integral       g = p * (float)(1.0 / 255.0) + 0.0f, a serial f32 running sum along each row, then I[r] = rs[r] + I[r - 1]
                 (np.cumsum with dtype float32 is np.add.accumulate: one add after the other, checked against a plain loop in
                 tests/test_surfdet_model_cpu.py);
  geometry       the layer table of buildResponseMap from integer divisions;
  responses      buildResponseLayer / BoxIntegral, operand by operand;
  extrema        getIpoints / isExtremum, the layers read through getResponse's width quotient;
  interpolate    deriv3D / hessian3D in f64 and x = -inv(H) dD with the closed-form adjugate inverse below (inv3): the one
                 definition the library, the fixture tool's stand-in and this model share.
detect() returns what modsx_debug_surfdet reports, plus counters of what the case exercised."""
import hashlib

import numpy as np

F = np.float32
D = np.float64
FILTERS = (9, 15, 21, 27, 39, 51, 75, 99, 147, 195, 291, 387)
FILTER_MAP = ((0, 1, 2, 3), (1, 3, 4, 5), (3, 5, 6, 7), (5, 7, 8, 9), (7, 9, 10, 11))
INI = dict(octaves=4, intervals=4, init_sample=2, thresh=0.0004)      # the [SURF] section of every shipped config file
DET_SURF = 6


def normalise(octaves=4, intervals=4, init_sample=2, thresh=0.0004):
    """FastHessian::saveParameters -> (octaves, intervals, init_sample, thresh f32)"""
    thresh = F(thresh)
    return (octaves if 0 < octaves <= 4 else 5, intervals if 0 < intervals <= 4 else 4,
            init_sample if 0 < init_sample <= 6 else 2, thresh if thresh >= 0 else F(0.0004))


def geometry(rows, cols, **params):
    """[(width, height, step, filter)] of buildResponseMap; ValueError where the reference's assert(width > 0 && height > 0) fires"""
    octaves, _, s, _ = normalise(**params)
    w, h = cols // s, rows // s
    out = []
    for o in range(octaves):
        d = 1 << o
        if w // d <= 0 or h // d <= 0:
            raise ValueError("a response layer of %d x %d" % (w // d, h // d))
        out += [(w // d, h // d, s * d, f) for f in (FILTERS[:4] if o == 0 else FILTERS[2 + 2 * o:4 + 2 * o])]
    return out


def integral(img, row_sum="serial"):
    g = np.asarray(img, F) * F(1.0 / 255.0) + F(0.0)
    if row_sum == "serial":
        rs = np.cumsum(g, axis=1, dtype=F)
    else:           # a log-step (tree) scan: what the kernels must NOT do
        rs = g.copy()
        k = 1
        while k < rs.shape[1]:
            nxt = rs.copy()
            nxt[:, k:] = rs[:, k:] + rs[:, :-k]
            rs, k = nxt, 2 * k
    return np.cumsum(rs, axis=0, dtype=F)


def _box(I, row, col, rows, cols, stats):
    H, W = I.shape
    r1, c1 = np.minimum(row, H) - 1, np.minimum(col, W) - 1
    r2, c2 = np.minimum(row + rows, H) - 1, np.minimum(col + cols, W) - 1

    def at(r, c):
        r, c = np.broadcast_arrays(r, c)
        return np.where((r >= 0) & (c >= 0), I[np.maximum(r, 0), np.maximum(c, 0)], F(0))
    v = at(r1, c1) - at(r1, c2) - at(r2, c1) + at(r2, c2)
    assert v.dtype == F
    if stats is not None:
        stats["top"] += int((r1 < 0).sum()); stats["left"] += int((c1 < 0).sum())
        stats["bottom"] += int((row + rows > H).sum()); stats["right"] += int((col + cols > W).sum())
        stats["max0"] += int((v < 0).sum())
    return np.where(v > 0, v, F(0))          # std::max(0.f, v): v only where 0.f < v


def response_layer(I, w, h, step, filt, stats=None):
    """buildResponseLayer -> (responses [h][w] f32, laplacian [h][w] u8)"""
    b, l = (filt - 1) // 2, filt // 3
    inv = F(1.0) / F(filt * filt)
    r, c = (np.arange(h) * step)[:, None], (np.arange(w) * step)[None, :]
    box = lambda *a: _box(I, *a, stats)                    # noqa: E731
    Dxx = box(r - l + 1, c - b, 2 * l - 1, filt) - box(r - l + 1, c - l // 2, 2 * l - 1, l) * F(3)
    Dyy = box(r - b, c - l + 1, filt, 2 * l - 1) - box(r - l // 2, c - l + 1, l, 2 * l - 1) * F(3)
    Dxy = box(r - l, c + 1, l, l) + box(r + 1, c - l, l, l) - box(r - l, c - l, l, l) - box(r + 1, c + 1, l, l)
    Dxx, Dyy, Dxy = Dxx * inv, Dyy * inv, Dxy * inv
    resp = Dxx * Dyy - F(0.81) * Dxy * Dxy
    assert resp.dtype == F and resp.shape == (h, w)
    return resp, (Dxx + Dyy >= 0).astype(np.uint8)


def inv3(S):
    """The specification of the 3 x 3 inverse (the reference calls cvInvert(., ., CV_SVD)): the adjugate over the determinant in
    f64, in exactly this order; all zeros where the determinant is 0 or not finite.  S: [n][9] row major -> [n][9]"""
    S = [S[:, k] for k in range(9)]
    with np.errstate(all="ignore"):
        d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
        ok = (d != 0) & np.isfinite(d)
        d = 1.0 / np.where(ok, d, 1.0)
        t = [(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
             (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
             (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d]
    return np.stack([np.where(ok, v, 0.0) for v in t], axis=1)


def _quotient(src, t, nominal):
    return (src[0] // t[0]) if not nominal else (t[2] // src[2])


def detect(img, row_sum="serial", nominal_quotient=False, **params):
    """-> dict(params, layers, integral, resp, lap, extrema [n][4] (o, i, r, c), dD [n][3], H [n][6] (dxx, dxy, dxs, dyy, dys,
    dss), x [n][3] (xc, xr, xi), accepted [n], laplacian [n], points [k][3] f32 (x, y, scale), points_lap [k], point_of [k] (the
    extremum a point came from), stats)"""
    img = np.asarray(img, F)
    octaves, intervals, s, thresh = normalise(**params)
    layers = geometry(img.shape[0], img.shape[1], **params)
    stats = dict(top=0, left=0, bottom=0, right=0, max0=0)
    I = integral(img, row_sum)
    planes = [response_layer(I, *L, stats) for L in layers]
    resp, lap = [p[0] for p in planes], [p[1] for p in planes]
    ext, dDs, Hs, xs, laps, pts = [], [], [], [], [], []
    quotients = set()
    for o in range(octaves):
        for i in (0, 1):
            ib, im, it = FILTER_MAP[o][i:i + 3]
            Lb, Lm, Lt = layers[ib], layers[im], layers[it]
            tw, th, tstep, tf = Lt
            border = (tf + 1) // (2 * tstep)
            rr, cc = np.arange(border + 1, th - border), np.arange(border + 1, tw - border)
            if len(rr) == 0 or len(cc) == 0:
                continue
            sb, sm = _quotient(Lb, Lt, nominal_quotient), _quotient(Lm, Lt, nominal_quotient)
            quotients.update(((Lb[0], tw, sb), (Lm[0], tw, sm)))
            T = lambda r, c: resp[it][r, c]                         # noqa: E731
            M = lambda r, c: resp[im][sm * r, sm * c]               # noqa: E731
            B = lambda r, c: resp[ib][sb * r, sb * c]               # noqa: E731
            R, Cc = rr[:, None], cc[None, :]
            cand = M(R, Cc)
            keep = ~(cand < thresh)
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    keep &= ~(T(R + dr, Cc + dc) >= cand)
                    if dr or dc:
                        keep &= ~(M(R + dr, Cc + dc) >= cand)
                    keep &= ~(B(R + dr, Cc + dc) >= cand)
            kr, kc = np.nonzero(keep)                               # raster order of the t layer
            if len(kr) == 0:
                continue
            r, c = rr[kr], cc[kc]
            f64 = lambda v: v.astype(D)                             # noqa: E731
            dx = f64(M(r, c + 1) - M(r, c - 1)) / 2.0
            dy = f64(M(r + 1, c) - M(r - 1, c)) / 2.0
            ds = f64(T(r, c) - B(r, c)) / 2.0
            v = f64(M(r, c))
            dxx = f64(M(r, c + 1) + M(r, c - 1)) - 2 * v
            dyy = f64(M(r + 1, c) + M(r - 1, c)) - 2 * v
            dss = f64(T(r, c) + B(r, c)) - 2 * v
            dxy = f64(M(r + 1, c + 1) - M(r + 1, c - 1) - M(r - 1, c + 1) + M(r - 1, c - 1)) / 4.0
            dxs = f64(T(r, c + 1) - T(r, c - 1) - B(r, c + 1) + B(r, c - 1)) / 4.0
            dys = f64(T(r + 1, c) - T(r - 1, c) - B(r + 1, c) + B(r - 1, c)) / 4.0
            Hi = inv3(np.stack([dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss], axis=1))
            with np.errstate(all="ignore"):
                x = np.stack([-1.0 * (Hi[:, 3 * k] * dx + Hi[:, 3 * k + 1] * dy + Hi[:, 3 * k + 2] * ds) for k in range(3)], axis=1)
            xc, xr, xi = x[:, 0], x[:, 1], x[:, 2]
            ok = (np.abs(xi) < 0.5) & (np.abs(xr) < 0.5) & (np.abs(xc) < 0.5)
            fstep = Lm[3] - Lb[3]
            assert fstep > 0 and tf - Lm[3] == fstep
            p = np.stack([((c + xc) * tstep).astype(F), ((r + xr) * tstep).astype(F),
                          (D(F(0.1333)) * (Lm[3] + xi * fstep)).astype(F)], axis=1)
            ext.append(np.stack([np.full(len(r), o), np.full(len(r), i), r, c], axis=1).astype(np.int32))
            dDs.append(np.stack([dx, dy, ds], axis=1)); Hs.append(np.stack([dxx, dxy, dxs, dyy, dys, dss], axis=1))
            xs.append(x); laps.append(lap[im][sm * r, sm * c].astype(np.int32)); pts.append((ok, p))
    cat = lambda a, shape, dt: np.concatenate(a) if a else np.zeros(shape, dt)          # noqa: E731
    accepted = cat([ok for ok, _ in pts], (0,), bool)
    allp = cat([p for _, p in pts], (0, 3), F)
    laplacian = cat(laps, (0,), np.int32)
    return dict(params=(octaves, intervals, s, thresh), layers=layers, integral=I, resp=resp, lap=lap,
                extrema=cat(ext, (0, 4), np.int32), dD=cat(dDs, (0, 3), D), H=cat(Hs, (0, 6), D), x=cat(xs, (0, 3), D),
                accepted=accepted, laplacian=laplacian, points=allp[accepted], points_lap=laplacian[accepted],
                point_of=np.nonzero(accepted)[0], stats=stats, quotients=sorted(quotients))


def keypoints(points, dtype):
    """the det_kp of the reference's SURF branch (imagerepresentation.cpp:1065-1075): orientation 0"""
    k = np.zeros(len(points), dtype)
    k["x"], k["y"], k["s"] = points[:, 0].astype(D), points[:, 1].astype(D), points[:, 2].astype(D)
    k["a11"], k["a12"], k["a21"], k["a22"] = np.cos(0.0), np.sin(0.0), -np.sin(0.0), np.cos(0.0)
    return k


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def sample_index(n, seed=4711, k=64):
    """the k seeded flat indices at which the fixture samples a plane of n values"""
    return np.random.default_rng(seed + n).integers(0, n, k)
