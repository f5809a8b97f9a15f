"""Inputs of the external affine adaptation tests (tests/test_affshape_cases_cpu.py, tests/test_gpu_affshape.py): three small f32
images and one region list per image.  tests/test_affshape_cases_cpu.py proves from the oracle's reports that they reach what
they claim.  No GPU in here.

Images (`images(oracle)`), rows x cols:
  0  48 x 64   blobs
  1  61 x 97   a constant band (all gradients 0: the NaN exit), blobs, a ridge band (one gradient direction: the anisotropy exit)
  2  19 x 23   blobs; smaller than most windows' reach
Regions (`regions()`, one REGION array per image): positions uniform from 2 px outside one side to 2 px outside the other, scales
1.6 f (as f32 numbers, see tests/affshape_model.py) with f in SCALES, some of them negative, and three kinds of input matrix:
identity, rotated anisotropic, and a small multiple of a rotation (such a region passes the up-front border test close to the
border, where the loop's own windows -- which start from the identity -- leave the image).  Planted among them (PLANTED names them,
`planted()` gives image, index): centres next to each of the four sides, the pairs that the identity and the own matrix judge
differently, and scales whose 10 * ratio lies one f32 step below and on an integer (odd, even and 1, the step res = 0 -> 1) at
positions where the border test's answer follows res.
"""
import numpy as np

from mods_amd import synthetic

SHAPES = ((48, 64), (61, 97), (19, 23))          # rows, cols
SCALES = (0.12, 0.2, 0.3, 0.45, 0.6, 0.8, 1.0, 1.3)
PER_IMAGE = (110, 130, 60)
INTERIOR = (90, 70)                              # images 0 and 1: further regions well inside the blobs
SEED = 7311
FLAT_COLS, RIDGE_COL0 = 30, 68                   # image 1: columns [0, 30) constant, [68, 97) ridge
KEYPOINT = np.dtype([("x", "f8"), ("y", "f8"), ("a11", "f8"), ("a12", "f8"), ("a21", "f8"), ("a22", "f8"),
                     ("s", "f8"), ("response", "f8"), ("octave_number", "i4"), ("pyramid_scale", "f8"),
                     ("sub_type", "i4")], align=True)
REGION = np.dtype([("img_id", "i4"), ("img_reproj_id", "i4"), ("id", "i4"), ("parent_id", "i4"), ("type", "i4"),
                   ("det_kp", KEYPOINT), ("reproj_kp", KEYPOINT)], align=True)
SIGMA = np.float32(1.6)

_images = None
_regions = None
_planted = {}


def images(oracle):
    """the three images, f32, built once"""
    global _images
    if _images is None:
        out = []
        for (r, c), nb, seed in zip(SHAPES, (40, 70, 8), (5101, 5102, 5103)):
            out.append(np.array(oracle.gaussian_blur(synthetic.blob_image(r, c, nb, seed), 1.0), np.float32))
        r, c = SHAPES[1]
        rs = np.random.RandomState(5104)
        yy, xx = np.mgrid[0:r, 0:c].astype(np.float64)
        ridge = 128.0 + 70.0 * np.sin(0.55 * xx + 0.08 * yy) + rs.uniform(-1.5, 1.5, xx.shape)
        ridge = np.array(oracle.gaussian_blur(ridge.astype(np.float32), 1.2), np.float32)
        out[1][:, :FLAT_COLS] = 90.0
        out[1][:, RIDGE_COL0:] = ridge[:, RIDGE_COL0:]
        _images = [np.ascontiguousarray(p, np.float32) for p in out]
        for p in _images:
            p.setflags(write=False)
    return _images


def f32_scale(f):
    """1.6 f as an f32 number (a double that an f32 holds exactly)"""
    return float(np.float32(np.float32(1.6) * np.float32(f)))


def scale_at_step(m):
    """-> (s_below, s_on): f32 scales whose ratio (float)(s / (double)1.6f) gives 10 * ratio just below the integer m (res = m - 1)
    and on or just above it (res = m), neighbours in the list of f32 scales"""
    s = np.float32(np.float32(1.6) * np.float32(m) / np.float32(10.0))
    for _ in range(8):
        s = np.nextafter(s, np.float32(0))
    prev = None
    for _ in range(32):
        ratio = np.float32(np.float64(s) / np.float64(SIGMA))
        res = int(np.trunc(10.0 * np.float64(ratio)))
        if res == m:
            assert prev is not None
            return float(prev), float(s)
        assert res == m - 1
        prev = s
        s = np.nextafter(s, np.float32(1e9))
    raise AssertionError(m)


def _reg(x, y, s, A=(1.0, 0.0, 0.0, 1.0)):
    return (float(x), float(y), float(s), float(A[0]), float(A[1]), float(A[2]), float(A[3]))


def _rot(phi, k1=1.0, k2=1.0):
    c, s = np.cos(phi), np.sin(phi)
    R = np.array([[c, -s], [s, c]])
    return tuple((R @ np.diag([k1, k2])).reshape(4))


def _random(rs, rows, cols, count):
    out = []
    for _ in range(count):
        x, y = rs.uniform(-2.0, cols + 2.0), rs.uniform(-2.0, rows + 2.0)
        s = f32_scale(SCALES[rs.randint(0, len(SCALES))])
        if rs.uniform() < 0.08:
            s = -s
        kind = rs.randint(0, 4)
        if kind <= 1:
            A = (1.0, 0.0, 0.0, 1.0)
        elif kind == 2:
            A = _rot(rs.uniform(0, np.pi), rs.uniform(0.6, 2.0), rs.uniform(0.6, 2.0))
        else:
            A = _rot(rs.uniform(0, np.pi), rs.uniform(0.05, 0.4), rs.uniform(0.05, 0.4))
        out.append(_reg(x, y, s, A))
    return out


def _planted_for(rows, cols):
    """name -> region tuple, for one image"""
    p = {}
    mx, my = 0.5 * cols, 0.5 * rows
    s5 = f32_scale(0.5)                      # ratio 0.5, res 5, half 3
    # one side each: the centre 2.5 px from that side, far from the others (the corner conditions of interpolateCheckBorders)
    p["left"] = _reg(2.5, my, s5)
    p["top"] = _reg(mx, 2.5, s5)
    p["right"] = _reg(cols - 3.5, my, s5)
    p["bottom"] = _reg(mx, rows - 3.5, s5)
    # judged differently by the identity and by the region's own matrix
    p["identity passes, own matrix refused"] = _reg(mx, 6.5, s5, _rot(0.7, 0.5, 2.6))
    p["identity refused, own matrix passes"] = _reg(mx, 3.5, s5, _rot(0.7, 0.2, 0.3))
    # 10 * ratio one step below / on an integer, where the border test follows res: centre at 1 + h + 0.5 from the left side passes
    # with half width h and not with h + 1 (res 0 -> 1: h = 0; res 6 -> 7: h = 3); even steps (res 1 -> 2, 7 -> 8) keep the half width
    for m, x in ((1, 1.5), (2, 2.5), (7, 4.5), (8, 5.5)):
        below, on = scale_at_step(m)
        p["step %d below" % m] = _reg(x, my, below)
        p["step %d on" % m] = _reg(x, my, on)
    p["negative scale"] = _reg(mx, my, -f32_scale(0.3))
    return p


PLANTED = tuple(_planted_for(40, 40).keys())


def regions():
    """-> [REGION array per image]: the whole case list; id = index in the image's list, type = 6 (SURF's detector type)"""
    global _regions
    if _regions is None:
        rs = np.random.RandomState(SEED)
        out = []
        for i, ((rows, cols), count) in enumerate(zip(SHAPES, PER_IMAGE)):
            lst = _random(rs, rows, cols, count)
            if i == 1:   # more of them inside the constant band and the ridge band
                for _ in range(25):
                    lst.insert(rs.randint(0, len(lst)), _reg(rs.uniform(9, FLAT_COLS - 9), rs.uniform(9, rows - 9), f32_scale(0.3)))
                for _ in range(40):
                    lst.insert(rs.randint(0, len(lst)), _reg(rs.uniform(RIDGE_COL0 + 4, cols - 8), rs.uniform(8, rows - 8),
                                                              f32_scale(SCALES[rs.randint(1, 5)])))
            if i < 2:    # regions that can converge: windows of the first iteration inside the blobs, any kind of input matrix
                x0, x1 = (14.0, cols - 14.0) if i == 0 else (FLAT_COLS + 10.0, RIDGE_COL0 - 10.0)
                for _ in range(INTERIOR[i]):
                    A = (1.0, 0.0, 0.0, 1.0) if rs.uniform() < 0.4 else _rot(rs.uniform(0, np.pi), rs.uniform(0.5, 1.6), rs.uniform(0.5, 1.6))
                    lst.insert(rs.randint(0, len(lst)), _reg(rs.uniform(x0, x1), rs.uniform(14.0, rows - 14.0),
                                                              f32_scale(SCALES[rs.randint(4, 8)]), A))
            planted = _planted_for(rows, cols)
            step = max(1, len(lst) // len(planted))
            for j, (name, t) in enumerate(planted.items()):
                lst.insert(min(len(lst), j * (step + 1)), t)
            where = {}
            for name, t in planted.items():
                where[name] = lst.index(t)
            _planted[i] = where
            a = np.zeros(len(lst), REGION)
            a["img_id"], a["type"], a["id"] = i, 6, np.arange(len(lst))
            for j, f in enumerate(("x", "y", "s", "a11", "a12", "a21", "a22")):
                a["det_kp"][f] = [t[j] for t in lst]
            a["det_kp"]["response"] = rs.uniform(0.0, 1.0, len(lst))
            a["reproj_kp"] = a["det_kp"]
            a.setflags(write=False)
            out.append(a)
        _regions = out
    return _regions


def planted(img, name):
    """index of a planted region in image img's list"""
    regions()
    return _planted[img][name]


_expected = {}


def expected(oracle, **params):
    """[(out regions, report)] per image: tests/affshape_model.run on the case list under the given parameters, cached"""
    from tests import affshape_model
    key = tuple(sorted(params.items()))
    if key not in _expected:
        _expected[key] = [affshape_model.run(oracle, im, r, **params) for im, r in zip(images(oracle), regions())]
    return _expected[key]
