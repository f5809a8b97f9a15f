#!/usr/bin/env python3
"""Records what the reference's OpenSURF detector computes on the images of tests/surfdet_cases.py: tests/golden/surfdet_ref.npz,
the golden data of tests/test_surfdet_model_cpu.py.  Run on a development machine that has the reference's sources; needs a C++
compiler, no GPU and no OpenCV:
    python tools/make_surfdet_fixture.py <reference root> tests/golden/surfdet_ref.npz
The reference's opensurf/fasthessian.cpp and opensurf/integral.cpp are compiled as they are, with the reference's own flags (-O3
-ftree-vectorize -funroll-loops -ansi, then -std=c++11; no fast-math, no -march), into a temporary directory, against the
stand-in opencv/cv.h and the driver of tools/surfdet_standin/, and driven through ctypes.  The stand-in header holds the CvMat
helpers and the adjugate cvInvert / cvGEMM that specify the one step OpenCV would run; the driver restates getGray and the few
lines of the SURF branch.  Per case the fixture holds the Ipoint list (x, y, scale, laplacian), the raw extremum list (o, i, r, c),
the layer table, a SHA-256 digest and 64 seeded samples of the integral image and of every response plane, a digest of every
laplacian plane, and the whole planes of the two smallest cases.  Nothing of the reference and nothing compiled from it is
written to the repository."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import surfdet_cases  # noqa: E402
import surfdet_model as M  # noqa: E402

STANDIN = os.path.join(ROOT, "tools", "surfdet_standin")
FLAGS = ["-O3", "-ftree-vectorize", "-funroll-loops", "-ansi", "-std=c++11", "-fPIC"]


def build(ref_root, tmp):
    cxx = os.environ.get("CXX", "c++")
    inc = ["-I" + STANDIN, "-I" + os.path.join(ref_root, "opensurf")]
    so = os.path.join(tmp, "libsurfdetref.so")
    subprocess.check_call([cxx] + FLAGS + ["-shared"] + inc +
                          [os.path.join(ref_root, "opensurf", "fasthessian.cpp"), os.path.join(ref_root, "opensurf", "integral.cpp"),
                           os.path.join(STANDIN, "driver.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.surfdet_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def run(lib, img, octaves, intervals, init_sample, thresh, cap_pts=1 << 20):
    """-> dict(integral, layers, resp, lap, points, points_lap, extrema) of the compiled reference"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    img = np.ascontiguousarray(img, np.float32)
    rows, cols = img.shape
    cap = 6 * rows * cols + 64
    integral, layers = np.zeros((rows, cols), np.float32), np.zeros((12, 4), np.int32)
    resp, lap = np.zeros(cap, np.float32), np.zeros(cap, np.uint8)
    pts, plap, ext = np.zeros((cap_pts, 3), np.float32), np.zeros(cap_pts, np.int32), np.zeros((cap_pts, 4), np.int32)
    counts = np.zeros(4, np.int64)
    rc = lib.surfdet_ref(p(img), rows, cols, int(octaves), int(intervals), int(init_sample), C.c_float(thresh), p(integral), p(layers),
                         p(resp), p(lap), cap, p(pts), p(plap), p(ext), cap_pts, p(counts))
    assert rc == 0, (rc, counts)
    nl, _, npts, next_ = (int(v) for v in counts)
    layers = layers[:nl]
    ofs = np.concatenate([[0], np.cumsum(layers[:, 0].astype(np.int64) * layers[:, 1])])
    planes = [resp[ofs[k]:ofs[k + 1]].reshape(layers[k, 1], layers[k, 0]).copy() for k in range(nl)]
    laps = [lap[ofs[k]:ofs[k + 1]].reshape(layers[k, 1], layers[k, 0]).copy() for k in range(nl)]
    return dict(integral=integral, layers=layers, resp=planes, lap=laps, points=pts[:npts].copy(), points_lap=plap[:npts].copy(),
                extrema=ext[:next_].copy())


def record(ref):
    """what the fixture keeps of one run"""
    planes = [ref["integral"]] + ref["resp"]
    return dict(points=ref["points"], points_lap=ref["points_lap"], extrema=ref["extrema"], layers=ref["layers"],
                digests=np.stack([M.digest(a) for a in planes]), lap_digests=np.stack([M.digest(a) for a in ref["lap"]]),
                samples=np.stack([a.reshape(-1)[M.sample_index(a.size)] for a in planes]))


def main(ref_root, out):
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref_root, tmp)
        names = surfdet_cases.names()
        data = dict(names=np.array(names))
        for k, (name, img, par) in enumerate(surfdet_cases.cases()):
            ref = run(lib, img, par["octaves"], par["intervals"], par["init_sample"], par["thresh"])
            for key, v in record(ref).items():
                data["c%02d_%s" % (k, key)] = v
            if name in surfdet_cases.WHOLE_PLANES:
                data["c%02d_integral" % k] = ref["integral"]
                for j, (a, b) in enumerate(zip(ref["resp"], ref["lap"])):
                    data["c%02d_resp_%d" % (k, j)], data["c%02d_lap_%d" % (k, j)] = a, b
            print("%-24s layers %2d extrema %6d points %6d" % (name, len(ref["layers"]), len(ref["extrema"]), len(ref["points"])))
    np.savez_compressed(out, **data)
    print("cases", len(names), "->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
