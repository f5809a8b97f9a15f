"""ctypes binding of the CPU oracle (oracle/liboracle.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py.  The product (mods_amd/) never imports this.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

KEYPOINT = np.dtype([("x", "f8"), ("y", "f8"), ("a11", "f8"), ("a12", "f8"), ("a21", "f8"), ("a22", "f8"),
                     ("s", "f8"), ("response", "f8"), ("octave_number", "i4"), ("pyramid_scale", "f8"),
                     ("sub_type", "i4")], align=True)
REGION = np.dtype([("img_id", "i4"), ("img_reproj_id", "i4"), ("id", "i4"), ("parent_id", "i4"), ("type", "i4"),
                   ("det_kp", KEYPOINT), ("reproj_kp", KEYPOINT)], align=True)
SSKP = np.dtype([("octave", "i4"), ("level", "i4"), ("r0", "i4"), ("c0", "i4"), ("r", "i4"), ("c", "i4"),
                 ("type", "i4"), ("pad", "i4"), ("b0", "f4"), ("b1", "f4"), ("b2", "f4"), ("val", "f4"),
                 ("x", "f4"), ("y", "f4"), ("s", "f4"), ("pixelDistance", "f4")], align=True)
TENT = np.dtype([("q", "i4"), ("t0", "i4"), ("tj", "i4"), ("t1", "i4"), ("d1", "f8"), ("d2", "f8"),
                 ("d2by2ndcl", "f8"), ("ratio", "f8")], align=True)
assert KEYPOINT.itemsize == 88 and REGION.itemsize == 200 and SSKP.itemsize == 64 and TENT.itemsize == 48


class HessAffParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("mode", C.c_int), ("reg_number", C.c_int),
                ("rel_threshold", C.c_float), ("rel_reg_number", C.c_float), ("numberOfScales", C.c_int),
                ("initialSigma", C.c_float), ("edgeEigenValueRatio", C.c_double), ("border", C.c_int),
                ("maxIterations", C.c_int), ("convergenceThreshold", C.c_float), ("smmWindowSize", C.c_int),
                ("affInitialSigma", C.c_float), ("doBaumberg", C.c_int), ("detectorType", C.c_int)]


class View(C.Structure):
    _fields_ = [("zoom", C.c_double), ("tilt", C.c_double), ("phi", C.c_double), ("InitSigma", C.c_double),
                ("doBlur", C.c_int)]


_REF_MSER_SO = os.path.join(_HERE, "_ref", "libmser_ref.so")
_REF_HESSAFF_SO = os.path.join(_HERE, "_ref", "libhessaff_ref.so")


def build(force=False):
    so = os.path.join(_HERE, "liboracle.so")
    srcs = [os.path.join(_HERE, f) for f in os.listdir(_HERE) if f.endswith((".cpp", ".hpp", ".h", ".c"))]
    stale = (not os.path.exists(so)) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", _HERE, "liboracle.so"], stdout=subprocess.DEVNULL)
    # the reference's own degensac, MSER and helpers / SIFT / affine shape, compiled in place where its sources are (`make ref`
    # builds what is missing of the three)
    want = [(os.path.join(_HERE, "_ref", "libdegensac_ref.so"), "/root/reference/degensac"), (_REF_MSER_SO, "/root/reference/detectors/mser"),
            (_REF_HESSAFF_SO, "/root/reference/detectors/affinedetectors")]
    if any(os.path.isdir(src) and (force or not os.path.exists(lib_)) for lib_, src in want):
        subprocess.check_call(["make", "-C", _HERE, "ref"], stdout=subprocess.DEVNULL)
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.orc_atan2lut.restype = C.c_float
        _lib.orc_atan2lut.argtypes = [C.c_float, C.c_float]
        _lib.orc_atan_lut.restype = C.POINTER(C.c_double)
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a, t=C.c_void_p):
    return a.ctypes.data_as(t)


def default_params(**kw):
    p = HessAffParams()
    lib().orc_default_hessaff_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def gray_from_bgr(bgr):
    bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
    out = np.empty(bgr.shape[:2], np.float32)
    lib().orc_gray_from_bgr_u8(_p(bgr), bgr.shape[0], bgr.shape[1], _p(out))
    return out


def gaussian_kernel(n, sigma):
    out = np.empty(n, np.float32)
    lib().orc_gaussian_kernel(C.c_int(n), C.c_double(sigma), _p(out))
    return out


def blur_ksize(sigma):
    return lib().orc_blur_ksize(C.c_float(sigma))


def gaussian_blur(img, sigma):
    img = _f32(img)
    out = np.empty_like(img)
    lib().orc_gaussian_blur(_p(img), img.shape[0], img.shape[1], C.c_float(sigma), _p(out))
    return out


def resize_half(img):
    img = _f32(img)
    r, c = C.c_int(), C.c_int()
    lib().orc_resize_half(_p(img), img.shape[0], img.shape[1], None, C.byref(r), C.byref(c))
    out = np.empty((r.value, c.value), np.float32)
    lib().orc_resize_half(_p(img), img.shape[0], img.shape[1], _p(out), C.byref(r), C.byref(c))
    return out


def hessian_response(img, norm):
    img = _f32(img)
    out = np.empty_like(img)
    lib().orc_hessian_response(_p(img), img.shape[0], img.shape[1], C.c_float(norm), _p(out))
    return out


def interpolate(img, ofsx, ofsy, a11, a12, a21, a22, rrows, rcols):
    img = _f32(img)
    out = np.empty((rrows, rcols), np.float32)
    t = lib().orc_interpolate(_p(img), img.shape[0], img.shape[1], C.c_float(ofsx), C.c_float(ofsy), C.c_float(a11),
                              C.c_float(a12), C.c_float(a21), C.c_float(a22), _p(out), rrows, rcols)
    return out, bool(t)


def atan_lut():
    return np.ctypeslib.as_array(lib().orc_atan_lut(), shape=(256,)).copy()


def atan2lut(y, x):
    return lib().orc_atan2lut(C.c_float(y), C.c_float(x))


def octave_levels(first, params, nlevels=5):
    first = _f32(first)
    blurs = np.empty((nlevels,) + first.shape, np.float32)
    resps = np.empty((nlevels,) + first.shape, np.float32)
    lib().orc_octave_levels(_p(first), first.shape[0], first.shape[1], C.byref(params), _p(blurs), _p(resps))
    return blurs, resps


def detect_scalespace(img, params, cap=400000):
    img = _f32(img)
    out = np.zeros(cap, SSKP)
    n = lib().orc_detect_scalespace(_p(img), img.shape[0], img.shape[1], C.byref(params), _p(out), cap)
    assert n <= cap
    return out[:n].copy()


SCAN_EXTREMUM = np.dtype([("level", "i4"), ("r0", "i4"), ("c0", "i4"), ("r", "i4"), ("c", "i4"), ("iters", "i4"), ("exit", "i4"),
                          ("type", "i4"), ("b0", "f4"), ("b1", "f4"), ("b2", "f4"), ("val", "f4")], align=True)
assert SCAN_EXTREMUM.itemsize == 48
# oracle.h: ORC_SCAN_*, in its order
SCAN_EXITS = ("accepted", "edge_high", "edge_negative", "nan", "border_right", "border_bottom", "border_left", "border_top",
              "offset", "value", "claimed")


def scan_levels(resps, blurs, params, claim=True):
    """orc_scan_levels: findLevelKeypoints + localizeKeypoint on the L = numberOfScales + 2 response / blur planes of one octave.
    -> (keypoints SSKP, report SCAN_EXTREMUM: one record per 3x3x3 extremum in scan order, `exit` an index into SCAN_EXITS)."""
    resps, blurs = _f32(resps), _f32(blurs)
    assert resps.ndim == 3 and resps.shape == blurs.shape
    L, rows, cols = resps.shape
    nrep = C.c_int(0)
    n = lib().orc_scan_levels(_p(resps), _p(blurs), L, rows, cols, C.byref(params), int(bool(claim)), None, 0, C.byref(nrep), None, 0)
    if n < 0:
        raise ValueError("orc_scan_levels refuses these planes / parameters")
    rep, out = np.zeros(max(nrep.value, 1), SCAN_EXTREMUM), np.zeros(max(n, 1), SSKP)
    n2 = lib().orc_scan_levels(_p(resps), _p(blurs), L, rows, cols, C.byref(params), int(bool(claim)), _p(rep), len(rep),
                               C.byref(nrep), _p(out), len(out))
    assert n2 == n
    return out[:n].copy(), rep[:nrep.value].copy()


def response(img, detector_type, norm):
    """ScaleSpaceDetector::Response (pyramid.cpp:132-175): 0 Hessian, 1 DoG, 2 Harris."""
    img = _f32(img)
    out = np.zeros_like(img)
    lib().orc_response(_p(img), img.shape[0], img.shape[1], int(detector_type), C.c_float(norm), _p(out))
    return out


def detect_hessaff(img, params, tilt=1.0, zoom=1.0, cap=400000):
    img = _f32(img)
    out = np.zeros(cap, KEYPOINT)
    n = lib().orc_detect_hessaff(_p(img), img.shape[0], img.shape[1], C.byref(params), C.c_double(tilt),
                                 C.c_double(zoom), _p(out), cap)
    assert n <= cap
    return out[:n].copy()


def find_affine_shape(blur, params, x, y, s, pixel_distance):
    blur = _f32(blur)
    u = np.zeros(4, np.float32)
    ok = lib().orc_find_affine_shape(_p(blur), blur.shape[0], blur.shape[1], C.byref(params), C.c_float(x),
                                     C.c_float(y), C.c_float(s), C.c_float(pixel_distance), _p(u))
    return ok, u


def find_affine_shape_batch(planes, plane_of, xyspd, params):
    """findAffineShape over a job list (planes: list of 2-D arrays; plane_of[k], xyspd[k] = x, y, s, pixelDistance of job k).
    -> dict(u [n, 4] f32, ok, iters, reason, touch): see orc_find_affine_shape_batch in oracle.h."""
    planes = [_f32(a) for a in planes]
    plane_of = np.ascontiguousarray(plane_of, np.int32)
    xyspd = np.ascontiguousarray(xyspd, np.float32).reshape(-1, 4)
    n = len(plane_of)
    assert len(xyspd) == n
    ptrs = (C.c_void_p * max(1, len(planes)))(*[a.ctypes.data for a in planes])
    rows = np.array([a.shape[0] for a in planes], np.int32)
    cols = np.array([a.shape[1] for a in planes], np.int32)
    u = np.zeros((n, 4), np.float32)
    ok, iters, reason, touch = (np.zeros(n, np.int32) for _ in range(4))
    rc = lib().orc_find_affine_shape_batch(ptrs, _p(rows), _p(cols), len(planes), _p(plane_of), _p(xyspd), n, C.byref(params),
                                           _p(u), _p(ok), _p(iters), _p(reason), _p(touch))
    assert rc == n, rc
    return dict(u=u, ok=ok, iters=iters, reason=reason, touch=touch)


def interpolate_check_borders(t):
    """interpolateCheckBorders for an [n, 9] array of (cols, rows, ofsx, ofsy, a11, a12, a21, a22, W) tuples -> bool [n]."""
    t = np.asarray(t)
    f = lib().orc_interpolate_check_borders
    f.argtypes = [C.c_int, C.c_int] + [C.c_float] * 6 + [C.c_int, C.c_int]
    return np.array([f(int(r[0]), int(r[1]), r[2], r[3], r[4], r[5], r[6], r[7], int(r[8]), int(r[8])) for r in t.tolist()], bool)


def interpolate_check_borders_wh(t):
    """interpolateCheckBorders for an [n, 10] array of (cols, rows, ofsx, ofsy, a11, a12, a21, a22, res_w, res_h) -> bool [n]"""
    f = lib().orc_interpolate_check_borders
    f.argtypes = [C.c_int, C.c_int] + [C.c_float] * 6 + [C.c_int, C.c_int]
    return np.array([f(int(r[0]), int(r[1]), r[2], r[3], r[4], r[5], r[6], r[7], int(r[8]), int(r[9])) for r in np.asarray(t).tolist()], bool)


def detect_affine_regions(kps, img_id=0, det_type=0):
    kps = np.ascontiguousarray(kps, KEYPOINT)
    out = np.zeros(len(kps), REGION)
    lib().orc_detect_affine_regions(_p(kps), len(kps), img_id, det_type, _p(out))
    return out


def detect_orientation(img, regs, mr_size=1.0, patch_size=41, half=0, max_ang=1, th=0.8, upright=0):
    img = _f32(img)
    regs = np.ascontiguousarray(regs, REGION)
    cap = max(1, len(regs) * max(1, 36 if max_ang < 0 else max_ang) + len(regs))
    out = np.zeros(cap, REGION)
    n = lib().orc_detect_orientation(_p(img), img.shape[0], img.shape[1], _p(regs), len(regs), C.c_double(mr_size),
                                     patch_size, half, max_ang, C.c_double(th), upright, _p(out), cap)
    assert n <= cap
    return out[:n].copy()


def dominant_angles(patch, half=0, th=0.8, max_angles=-1):
    patch = _f32(patch)
    out = np.zeros(40, np.float32)
    n = lib().orc_dominant_angles(_p(patch), patch.shape[0], half, C.c_double(th), max_angles, _p(out), 40)
    return out[:n].copy()


def reproject_regions(regs, H, w, h):
    regs = np.ascontiguousarray(regs, REGION).copy()
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    n = lib().orc_reproject_regions(_p(regs), len(regs), _p(H), w, h)
    return regs[:n].copy()


def reproject_regions_touch_boundary(regs, H, w, h, mr_size=3.0 * 3.0 ** 0.5):
    regs = np.ascontiguousarray(regs, REGION).copy()
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    n = lib().orc_reproject_regions_touch_boundary(_p(regs), len(regs), _p(H), w, h, C.c_double(mr_size))
    return regs[:n].copy()


def describe_regions(img, regs, mr_size=5.1962, patch_size=41, fast=0, photo_norm=1, rootsift=1, max_bin=0.2):
    img = _f32(img)
    regs = np.ascontiguousarray(regs, REGION)
    desc = np.zeros((len(regs), 128), np.float32)
    lib().orc_describe_regions(_p(img), img.shape[0], img.shape[1], _p(regs), len(regs), C.c_double(mr_size),
                               patch_size, fast, photo_norm, rootsift, C.c_double(max_bin), _p(desc))
    return desc


def extract_patch(img, reg, mr_size=5.1962, patch_size=41):
    img = _f32(img)
    reg = np.ascontiguousarray(reg, REGION).reshape(1)
    patch = np.zeros((patch_size, patch_size), np.float32)
    lib().orc_extract_patch(_p(img), img.shape[0], img.shape[1], _p(reg), C.c_double(mr_size), patch_size, _p(patch))
    return patch


def describe_patch(patch, photo_norm=1, rootsift=1, max_bin=0.2):
    p = _f32(patch).copy()
    desc = np.zeros(128, np.float32)
    lib().orc_describe_patch(_p(p), photo_norm, rootsift, C.c_double(max_bin), _p(desc))
    return desc, p


def knn_linear(d1, d2, nn=50):
    d1, d2 = _f32(d1), _f32(d2)
    idx = np.zeros((len(d1), nn), np.int32)
    dist = np.zeros((len(d1), nn), np.float32)
    lib().orc_knn_linear(_p(d1), len(d1), _p(d2), len(d2), d1.shape[1], nn, _p(idx), _p(dist))
    return idx, dist


def match_fginn(d1, d2, pos2, ratio=0.8, contrad_dist=30.0, nn=50):
    d1, d2 = _f32(d1), _f32(d2)
    pos2 = np.ascontiguousarray(pos2, np.float64)
    out = np.zeros(max(1, len(d1)), TENT)
    n = lib().orc_match_fginn(_p(d1), len(d1), _p(d2), len(d2), d1.shape[1] if len(d1) else 128, _p(pos2),
                              C.c_double(ratio), C.c_double(contrad_dist), nn, _p(out), len(out))
    return out[:n].copy()


def duplicate_filtering(pts, key, r=2.0, do_sort=True):
    pts = np.ascontiguousarray(pts, np.float64)
    key = np.ascontiguousarray(key, np.float64)
    T = len(pts)
    order = np.zeros(T, np.int32)
    keep = np.zeros(T, np.uint8)
    lib().orc_duplicate_filtering(_p(pts), _p(key), T, C.c_double(r), int(do_sort), _p(order), _p(keep))
    return order, keep.astype(bool)


def ref_available():
    return bool(lib().orc_ref_available())


def detect_msers(img, min_size=30, max_area=0.05, min_margin=8.0, relative=0, mode=0, reg_number=500, rel_threshold=-1.0,
                 rel_reg_number=-1.0, tilt=1.0, zoom=1.0):
    """DetectMSERs (extrema.cpp:284-473, doOnNormal); defaults = [MSER] of config_iter_mods_cviu.ini.
    The restatement (oracle_mser.cpp).  PINNED to the reference's own sources by tests/test_mser_ref_cpu.py (detect_msers_ref
    below, bit for bit on the nine fields DetectMSERs sets) for images of 64 pixels and more.  NOT pinned: images under 64
    pixels, which the reference cannot be handed, and the OpenCV-backed view synthesis that runs in front of MSER."""
    img = _f32(img)
    cap = 1 << 16
    while True:
        out = np.zeros(cap, KEYPOINT)
        n = lib().orc_detect_msers(_p(img), img.shape[0], img.shape[1], int(min_size), C.c_double(max_area),
                                   C.c_double(min_margin), int(relative), int(mode), int(reg_number),
                                   C.c_double(rel_threshold), C.c_double(rel_reg_number), C.c_double(tilt),
                                   C.c_double(zoom), _p(out), cap)
        if n <= cap:
            return out[:n].copy()
        cap = n


# ---- the reference's own MSER (oracle/_ref/libmser_ref.so: detectors/mser compiled in place, oracle/ref_mser_shim.cpp) ----
# The reference faults (SIGSEGV) on tiny images: every image tried with fewer than 30 pixels at the default min_size = 30 did, and
# every one tried with 30 or more ran.  64 is a MARGIN over that observed line of 30, not a measured quantity: nothing smaller is
# handed to the reference, so images under 64 pixels are the one MSER input class that stays checked against the restatement
# (detect_msers) alone.
# The cause behind that line, read from the code and then measured (84 x 1 at min_size 85 faults, at 84 it runs; 10 x 10 at 101
# faults, at 100 it runs): an image of fewer than min(10000, min_size) pixels never upgrades a component to a region, the root
# label is still a packed counter when GetExtrema (getExtrema.cpp:428-434) casts it to a t_region pointer and dereferences it.
# Such a call is refused below as well, whatever the image's size.
REF_MSER_MIN_PIXELS = 64
# the reference keeps its state in file-level statics (labels_ptr, g_cols, ...): one call at a time, whatever the thread
_ref_mser_lock = threading.Lock()
_ref_mser_lib = None


def ref_mser_available():
    build()
    return os.path.exists(_REF_MSER_SO)


def detect_msers_ref(img, min_size=30, max_area=0.05, min_margin=8.0, relative=0, mode=0, reg_number=500, rel_threshold=-1.0,
                     rel_reg_number=-1.0, tilt=1.0, zoom=1.0):
    """The reference's DetectMSERs (5-argument overload, extrema.cpp:284-473) on f32 pixels: its own (unsigned char) conversion,
    component tree, stability selection, boundaries, ellipses and export.  Same keywords and defaults as detect_msers.
    -> KEYPOINT records; octave_number and pyramid_scale, which the reference never writes, are zero."""
    global _ref_mser_lib
    img = _f32(img)
    if img.ndim != 2:
        raise ValueError("detect_msers_ref: a 2-d image is expected")
    if img.size < REF_MSER_MIN_PIXELS:
        raise ValueError("detect_msers_ref: the reference faults on tiny images; %d x %d is under the %d-pixel margin"
                         % (img.shape[0], img.shape[1], REF_MSER_MIN_PIXELS))
    if img.size < min(10000, int(min_size)):
        raise ValueError("detect_msers_ref: the reference faults when the image (%d pixels) is smaller than min(10000, min_size = %d)"
                         % (img.size, int(min_size)))
    with _ref_mser_lock:
        if _ref_mser_lib is None:
            if not ref_mser_available():
                raise RuntimeError("oracle/_ref/libmser_ref.so is not built: run `make -C oracle ref` where the reference is")
            L = C.CDLL(_REF_MSER_SO)
            L.refmser_detect.restype = C.c_int
            L.refmser_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                         C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int]
            _ref_mser_lib = L
        cap = 1 << 12
        while True:
            out9 = np.zeros((cap, 9), np.float64)
            n = _ref_mser_lib.refmser_detect(_p(img), img.shape[0], img.shape[1], int(relative), int(min_size), float(max_area),
                                             float(min_margin), int(mode), float(rel_threshold), int(reg_number),
                                             float(rel_reg_number), float(tilt), float(zoom), _p(out9), cap)
            if n <= cap:
                break
            cap = n
    out = np.zeros(n, KEYPOINT)
    for i, f in enumerate(MSER_FIELDS):
        out[f] = out9[:n, i]
    return out


# ---- the oracle's parts on their own (what tests/test_ref_pin_cpu.py compares with the reference's functions) ----
def gauss_mask(size):
    out = np.zeros((size, size), np.float32)
    lib().orc_gauss_mask(int(size), _p(out))
    return out


def circular_gauss_mask(rows, cols, sigma=0.0):
    out = np.zeros((rows, cols), np.float32)
    lib().orc_circular_gauss_mask(int(rows), int(cols), C.c_float(sigma), _p(out))
    return out


def photo_norm(patch, mask=None):
    """photometricallyNormalize -> (patch, sum, var); mask None: the circular mask DescribeRegions builds"""
    p = _f32(patch).copy()
    m = None if mask is None else _f32(mask)
    s, v = C.c_float(), C.c_float()
    lib().orc_photo_norm(_p(p), p.shape[0], p.shape[1], None if m is None else _p(m), C.byref(s), C.byref(v))
    return p, np.float32(s.value), np.float32(v.value)


def inv_sqrt(a, b, c):
    """invSqrt -> (a, b, c, l1, l2) f32"""
    abc, l = np.array([a, b, c], np.float32), np.zeros(2, np.float32)
    lib().orc_inv_sqrt(_p(abc), _p(l))
    return np.concatenate([abc, l])


def get_eigenvalues(a, b, c, d):
    """getEigenvalues -> (ok, l1, l2); l1, l2 are 0 when it returns false"""
    l = np.zeros(2, np.float32)
    ok = lib().orc_get_eigenvalues(C.c_float(a), C.c_float(b), C.c_float(c), C.c_float(d), _p(l))
    return bool(ok), l


def solve_linear3x3(A, b):
    """solveLinear3x3 -> (A, b) as it leaves them"""
    A, b = _f32(A).reshape(9).copy(), _f32(b).reshape(3).copy()
    lib().orc_solve_linear3x3(_p(A), _p(b))
    return A, b


def rectify(a4):
    a = np.array(a4, np.float64).reshape(4).copy()
    lib().orc_rectify(_p(a))
    return a


def compute_gradient(img):
    img = _f32(img)
    gx, gy = np.zeros_like(img), np.zeros_like(img)
    lib().orc_compute_gradient(_p(img), img.shape[0], img.shape[1], _p(gx), _p(gy))
    return gx, gy


def grad_mag_ori(img):
    """computeGradientMagnitudeAndOrientation: interior pixels, the frame is 0"""
    img = _f32(img)
    mag, ori = np.zeros_like(img), np.zeros_like(img)
    lib().orc_grad_mag_ori(_p(img), img.shape[0], img.shape[1], _p(mag), _p(ori))
    return mag, ori


def sift_histogram(patch):
    """SIFTDescriptor's 128-bin histogram before any norm, f64"""
    p = _f32(patch)
    raw = np.zeros(128, np.float64)
    lib().orc_sift_histogram(_p(p), _p(raw))
    return raw


# ---- the reference's own helpers.cpp / siftdesc.cpp / affine.cpp (oracle/_ref/libhessaff_ref.so, oracle/ref_hessaff_shim.cpp) ----
# Every ref_* function below returns what the reference's function of that name computes; RefRefused is raised where the shim
# refuses the call because the reference would read or write out of bounds, or reach a cv:: operation (see the shim's comment).
class RefRefused(ValueError):
    pass


_ref_hessaff_lib = None
_ref_hessaff_lock = threading.Lock()


def ref_hessaff_available():
    build()
    return os.path.exists(_REF_HESSAFF_SO)


def _rh():
    global _ref_hessaff_lib
    with _ref_hessaff_lock:
        if _ref_hessaff_lib is None:
            if not ref_hessaff_available():
                raise RuntimeError("oracle/_ref/libhessaff_ref.so is not built: run `make -C oracle ref` where the reference is")
            L = C.CDLL(_REF_HESSAFF_SO)
            f, i, v = C.c_float, C.c_int, C.c_void_p
            L.refhess_atan2lutff.restype = f
            L.refhess_atan2lutff.argtypes = [f, f, v]
            L.refhess_sift.argtypes = [v, i, C.c_double, i, v, v]
            L.refhess_photo_norm.argtypes = [v, i, i, v, v, v]
            L.refhess_circular_gauss_mask.argtypes = [i, i, f, v]
            L.refhess_gauss_mask.argtypes = [i, v]
            L.refhess_interpolate.argtypes = [v, i, i, f, f, f, f, f, f, v, i, i]
            L.refhess_check_borders.argtypes = [i, i, f, f, f, f, f, f, i, i]
            L.refhess_check_borders_mat.argtypes = [i, i, f, f, f, f, f, f, i, i]
            L.refhess_inv_sqrt.argtypes = [v, v]
            L.refhess_get_eigenvalues.argtypes = [f, f, f, f, v]
            L.refhess_solve_linear3x3.argtypes = [v, v]
            for n in ("refhess_rectify_f", "refhess_rectify_d", "refhess_rectify_dp"):
                getattr(L, n).argtypes = [v]
            L.refhess_compute_gradient.argtypes = [v, i, i, v, v]
            L.refhess_grad_mag_ori.argtypes = [v, i, i, v, v]
            L.refhess_find_affine_shape_batch.argtypes = [v, v, v, i, v, v, i, i, f, i, f, i, i, v, v, v]
            _ref_hessaff_lib = L
    return _ref_hessaff_lib


def _refused(rc, what):
    if rc < 0:
        raise RefRefused("%s: the shim refuses this call (%d)" % (what, rc))
    return rc


def ref_atan2lutff(y, x):
    """atan2LUTff(y, x) as f32; RefRefused where the reference would index outside ATAN_LUT"""
    r = C.c_int()
    out = _rh().refhess_atan2lutff(float(np.float32(y)), float(np.float32(x)), C.byref(r))
    if r.value:
        raise RefRefused("atan2LUTff(%r, %r) indexes outside the table" % (y, x))
    return np.float32(out)


def ref_sift(patch, desc_type=1, max_bin=0.2, route=None):
    """SIFTDescriptor on a 41 x 41 patch -> (desc f32 [128], raw f64 [128]).  desc_type 0 SIFT, 1 RootSIFT, 2 HalfSIFT,
    3 HalfRootSIFT (64 values, then zeros); raw = the public `vec` with doNorm = false.  route 0: operator() as DescribeRegions
    calls it; route 1: the Half types through the public SIFTnorm / RootSIFTnorm (the shim's comment says why HalfSIFT must);
    default: 1 for HalfSIFT, 0 otherwise."""
    p = _f32(patch)
    assert p.shape == (41, 41)
    route = (1 if desc_type == 2 else 0) if route is None else route
    desc, raw = np.zeros(128, np.float32), np.zeros(128, np.float64)
    _refused(_rh().refhess_sift(_p(p), int(desc_type), float(max_bin), int(route), _p(desc), _p(raw)), "SIFTDescriptor")
    return desc, raw


def ref_photo_norm(patch, mask=None):
    """photometricallyNormalize -> (patch, sum, var); mask None: computeCircularGaussMask(mask) of the patch's size"""
    p = _f32(patch).copy()
    m = None if mask is None else _f32(mask)
    s, v = C.c_float(), C.c_float()
    _refused(_rh().refhess_photo_norm(_p(p), p.shape[0], p.shape[1], None if m is None else _p(m), C.byref(s), C.byref(v)),
             "photometricallyNormalize")
    return p, np.float32(s.value), np.float32(v.value)


def ref_describe_patch(patch, photo_norm=1, desc_type=1, max_bin=0.2, route=None):
    """what DescribeRegions does with an extracted patch (synth-detection.hpp:225-229): photometricallyNormalize under the circular
    mask when photoNorm, then the descriptor -> (desc, raw, patch as the descriptor saw it)"""
    p = ref_photo_norm(patch)[0] if photo_norm else _f32(patch).copy()
    desc, raw = ref_sift(p, desc_type, max_bin, route)
    return desc, raw, p


def ref_circular_gauss_mask(rows, cols, sigma=0.0):
    out = np.zeros((rows, cols), np.float32)
    _refused(_rh().refhess_circular_gauss_mask(int(rows), int(cols), float(sigma), _p(out)), "computeCircularGaussMask")
    return out


def ref_gauss_mask(size):
    out = np.zeros((size, size), np.float32)
    _refused(_rh().refhess_gauss_mask(int(size), _p(out)), "computeGaussMask")
    return out


def ref_interpolate(img, ofsx, ofsy, a11, a12, a21, a22, rrows, rcols):
    img = _f32(img)
    out = np.zeros((rrows, rcols), np.float32)
    t = _refused(_rh().refhess_interpolate(_p(img), img.shape[0], img.shape[1], ofsx, ofsy, a11, a12, a21, a22, _p(out), rrows, rcols),
                 "interpolate")
    return out, bool(t)


def ref_interpolate_check_borders(t, mat=False):
    """interpolateCheckBorders for an [n, 10] array of (cols, rows, ofsx, ofsy, a11, a12, a21, a22, res_w, res_h) -> bool [n];
    mat = True: the cv::Mat overload (image and result given as Mats of those sizes), else the int overload"""
    L = _rh()
    out = np.zeros(len(t), bool)
    for k, r in enumerate(np.asarray(t, np.float64).tolist()):
        if mat:
            out[k] = L.refhess_check_borders_mat(int(r[1]), int(r[0]), r[2], r[3], r[4], r[5], r[6], r[7], int(r[9]), int(r[8]))
        else:
            out[k] = L.refhess_check_borders(int(r[0]), int(r[1]), r[2], r[3], r[4], r[5], r[6], r[7], int(r[8]), int(r[9]))
    return out


def ref_inv_sqrt(a, b, c):
    abc, l = np.array([a, b, c], np.float32), np.zeros(2, np.float32)
    _rh().refhess_inv_sqrt(_p(abc), _p(l))
    return np.concatenate([abc, l])


def ref_get_eigenvalues(a, b, c, d):
    l = np.zeros(2, np.float32)
    ok = _rh().refhess_get_eigenvalues(float(np.float32(a)), float(np.float32(b)), float(np.float32(c)), float(np.float32(d)), _p(l))
    return bool(ok), l


def ref_solve_linear3x3(A, b):
    A, b = _f32(A).reshape(9).copy(), _f32(b).reshape(3).copy()
    _rh().refhess_solve_linear3x3(_p(A), _p(b))
    return A, b


def ref_rectify(a4, overload="double"):
    """rectifyAffineTransformationUpIsUp: overload "float" (float &), "double" (double &) or "pointer" (double *)"""
    if overload == "float":
        a = np.array(a4, np.float32).reshape(4).copy()
        _rh().refhess_rectify_f(_p(a))
    else:
        a = np.array(a4, np.float64).reshape(4).copy()
        (_rh().refhess_rectify_d if overload == "double" else _rh().refhess_rectify_dp)(_p(a))
    return a


def ref_compute_gradient(img):
    img = _f32(img)
    gx, gy = np.zeros_like(img), np.zeros_like(img)
    _refused(_rh().refhess_compute_gradient(_p(img), img.shape[0], img.shape[1], _p(gx), _p(gy)), "computeGradient")
    return gx, gy


def ref_grad_mag_ori(img):
    img = _f32(img)
    mag, ori = np.zeros_like(img), np.zeros_like(img)
    _refused(_rh().refhess_grad_mag_ori(_p(img), img.shape[0], img.shape[1], _p(mag), _p(ori)), "computeGradientMagnitudeAndOrientation")
    return mag, ori


def ref_find_affine_shape_batch(planes, plane_of, xyspd, params, method=0):
    """AffineShape::findAffineShape through an AffineShapeCallback, over a job list laid out as for find_affine_shape_batch, with
    maxIterations, convergenceThreshold, smmWindowSize, affInitialSigma and doBaumberg of `params` (a HessAffParams).
    -> dict(hit [n] i32, u [n, 4] f32, iters [n] i32); u and iters are written for hits only (zeros / -1 elsewhere): the reference
    reports nothing about a keypoint that did not converge.  method != 0 (AFF_BMBRG_HESSIAN) is refused."""
    planes = [_f32(a) for a in planes]
    plane_of = np.ascontiguousarray(plane_of, np.int32)
    xyspd = np.ascontiguousarray(xyspd, np.float32).reshape(-1, 4)
    n = len(plane_of)
    assert len(xyspd) == n
    ptrs = (C.c_void_p * max(1, len(planes)))(*[a.ctypes.data for a in planes])
    rows = np.array([a.shape[0] for a in planes], np.int32)
    cols = np.array([a.shape[1] for a in planes], np.int32)
    hit, u, iters = np.zeros(n, np.int32), np.zeros((n, 4), np.float32), np.full(n, -1, np.int32)
    rc = _rh().refhess_find_affine_shape_batch(ptrs, _p(rows), _p(cols), len(planes), _p(plane_of), _p(xyspd), n, int(params.maxIterations),
                                               float(params.convergenceThreshold), int(params.smmWindowSize), float(params.affInitialSigma),
                                               int(params.doBaumberg), int(method), _p(hit), _p(u), _p(iters))
    _refused(rc, "findAffineShape")
    assert rc == n, rc
    return dict(hit=hit, u=u, iters=iters)


MSER_FIELDS = ("x", "y", "a11", "a12", "a21", "a22", "s", "response", "sub_type")    # what DetectMSERs sets, in the shim's order


def loransac_h(pts, laf1, laf2, err_threshold=3.0, confidence=0.99, max_samples=100000, lo=1, hlaf_coef=12.0,
               sym_check=1, seed=1, error_type=0):
    pts = np.ascontiguousarray(pts, np.float64)
    laf1 = np.ascontiguousarray(laf1, np.float64)
    laf2 = np.ascontiguousarray(laf2, np.float64)
    T = len(pts)
    H = np.zeros(9)
    Hraw = np.zeros(9)
    inl = np.zeros(max(T, 1), np.uint8)
    keep = np.zeros(max(T, 1), np.uint8)
    dout = np.zeros(3, np.int32)
    n = lib().orc_loransac_h(_p(pts), _p(laf1), _p(laf2), T, C.c_double(err_threshold), C.c_double(confidence),
                             max_samples, lo, C.c_double(hlaf_coef), sym_check, C.c_uint(seed), _p(H), _p(Hraw),
                             _p(inl), _p(keep), _p(dout), int(error_type))
    return dict(n=n, H=H.reshape(3, 3), Hraw=Hraw, inl=inl[:T].astype(bool), keep=keep[:T].astype(bool),
                samples=int(dout[0]), lo_count=int(dout[1]), ori_rejects=int(dout[2]))


def loransac_f(pts, laf1, laf2, err_threshold=4.0, confidence=0.99, max_samples=100000, lo=1, laf_coef=3.0,
               sym_check=1, error_type=0, seed=1):
    """LORANSACFiltering with useF = 1 (the reference's exp_ransacFcustom from oracle/_ref + F_LAF_check)."""
    pts = np.ascontiguousarray(pts, np.float64)
    laf1 = np.ascontiguousarray(laf1, np.float64)
    laf2 = np.ascontiguousarray(laf2, np.float64)
    T = len(pts)
    F = np.zeros(9)
    inl = np.zeros(max(T, 1), np.uint8)
    keep = np.zeros(max(T, 1), np.uint8)
    dout = np.zeros(3, np.int32)
    n = lib().orc_loransac_f(_p(pts), _p(laf1), _p(laf2), T, C.c_double(err_threshold), C.c_double(confidence),
                             max_samples, lo, C.c_double(laf_coef), sym_check, error_type, C.c_uint(seed), _p(F),
                             _p(inl), _p(keep), _p(dout))
    return dict(n=n, F=F.reshape(3, 3), inl=inl[:T].astype(bool), keep=keep[:T].astype(bool),
                samples=int(dout[0]), lo_count=int(dout[1]))


def warp_affine(img, M6, drows, dcols, border=128.0):
    img = _f32(img)
    M6 = np.ascontiguousarray(M6, np.float64).reshape(6)
    out = np.empty((drows, dcols), np.float32)
    lib().orc_warp_affine(_p(img), img.shape[0], img.shape[1], _p(M6), _p(out), drows, dcols, C.c_float(border))
    return out


def gaussian_blur_xy(img, kx, ky, sx, sy):
    img = _f32(img)
    out = np.empty_like(img)
    lib().orc_gaussian_blur_xy(_p(img), img.shape[0], img.shape[1], kx, ky, C.c_double(sx), C.c_double(sy), _p(out))
    return out


def make_view(tilt=1.0, phi=0.0, zoom=1.0, init_sigma=0.5, do_blur=1):
    v = View()
    v.zoom, v.tilt, v.phi, v.InitSigma, v.doBlur = zoom, tilt, phi, init_sigma, do_blur
    return v


def synth_view(gray, view):
    gray = _f32(gray)
    r, c = C.c_int(), C.c_int()
    H = np.zeros(9)
    lib().orc_synth_view(_p(gray), gray.shape[0], gray.shape[1], C.byref(view), None, C.byref(r), C.byref(c), _p(H))
    out = np.empty((r.value, c.value), np.float32)
    ident = lib().orc_synth_view(_p(gray), gray.shape[0], gray.shape[1], C.byref(view), _p(out), C.byref(r),
                                 C.byref(c), _p(H))
    return out, H.reshape(3, 3), bool(ident)


def set_vs_pars(scale_set, tilt_set, phi_base, init_sigma=0.5, do_blur=1, prev=None):
    """SetVSPars; prev is a python list of View that is extended in place (de-duplication across steps)."""
    prev = [] if prev is None else prev
    ss = np.ascontiguousarray(scale_set, np.float64)
    ts = np.ascontiguousarray(tilt_set, np.float64)
    cap = 4096
    par = (View * cap)()
    pv = (View * cap)(*prev)
    npv = C.c_int(len(prev))
    n = lib().orc_set_vs_pars(_p(ss), len(ss), _p(ts), len(ts), C.c_double(phi_base), C.c_double(init_sigma),
                              int(do_blur), par, cap, pv, C.byref(npv), cap)
    del prev[:]
    for i in range(npv.value):
        prev.append(make_view(pv[i].tilt, pv[i].phi, pv[i].zoom, pv[i].InitSigma, pv[i].doBlur))
    return [make_view(par[i].tilt, par[i].phi, par[i].zoom, par[i].InitSigma, par[i].doBlur) for i in range(n)]


def detect_describe_views(gray, views, params=None, ori=(1.0, 41, 1, 0.8), desc=(5.1962, 41, 0, 1, 1, 0.2), mser=None, threads=1,
                          descs=None):
    """The HessianAffine / MSER branch of SynthDetectDescribeKeypoints (imagerepresentation.cpp:603-2047): per view
    synthesise, detect, orient, reproject, describe; concatenate in view order with AddRegionsToList id re-basing
    (:588-600).  Returns (regions, descriptors).  threads > 1: the views run on a thread pool (the reference's `#pragma omp
    parallel for` over views, :612-622; ctypes releases the GIL), same result.
    descs = the step's descriptor list (types 0 SIFT, 1 RootSIFT, 2 HalfSIFT, 3 HalfRootSIFT; default [desc[4]]): the
    reference orients ONCE per step -- with doHalfSIFT = true as soon as one name contains "Half" (:693-706, 1259-1264) -- and
    describes every descriptor of the step on that oriented list (:1288-1296).  With `descs` the second return value is the
    list of descriptor arrays, one per entry."""
    gray = _f32(gray)
    params = params or default_params()
    types = [desc[4]] if descs is None else list(descs)
    half = 1 if any(t >= 2 for t in types) else 0

    def one(job):
        vi, v = job
        img, H, ident = synth_view(gray, v)
        vt, vz = (abs(v.tilt) if not ident else 1.0), (v.zoom if not ident else 1.0)
        if mser is not None:   # DetectAffineRegions(..., DET_MSER, DetectMSERs), imagerepresentation.cpp:1037
            k = detect_msers(img, tilt=vt, zoom=vz, **mser)
            regs = detect_affine_regions(k, img_id=0 if ident else vi, det_type=3)
        else:
            k = detect_hessaff(img, params, tilt=vt, zoom=vz)
            regs = detect_affine_regions(k, img_id=0 if ident else vi)
        ro = detect_orientation(img, regs, mr_size=ori[0], patch_size=ori[1], half=half, max_ang=ori[2], th=ori[3])
        rr = reproject_regions(ro, H.reshape(9), gray.shape[1], gray.shape[0])
        d = [describe_regions(img, rr, mr_size=desc[0], patch_size=desc[1], fast=desc[2], photo_norm=desc[3],
                              rootsift=t, max_bin=desc[5]) for t in types]
        return rr.copy(), d

    jobs = list(enumerate(views))
    if threads > 1 and len(jobs) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as pool:
            parts = list(pool.map(one, jobs))
    else:
        parts = [one(j) for j in jobs]
    all_regs, all_desc = [], []
    size = 0
    for rr, d in parts:
        rr["id"] += size
        rr["parent_id"] += size
        size += len(rr)
        all_regs.append(rr)
        all_desc.append(d)
    regs = np.concatenate(all_regs) if all_regs else np.zeros(0, REGION)
    per = [np.concatenate([d[k] for d in all_desc]) if all_desc else np.zeros((0, 128), np.float32) for k in range(len(types))]
    return regs, (per if descs is not None else per[0])
