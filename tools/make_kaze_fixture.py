#!/usr/bin/env python3
"""Records what the reference's AKAZE detector computes on the cases of tests/kaze_cases.py: tests/golden/kaze_ref.npz, the
golden data of tests/test_kaze_model_cpu.py.  Run on a development machine that has the reference's sources; needs a C++
compiler, no GPU and no OpenCV:
    python tools/make_kaze_fixture.py <reference root> tests/golden/kaze_ref.npz
The reference's akaze/src/lib/AKAZE.cpp, nldiffusion_functions.cpp and fed.cpp are compiled as they are, with the reference's own
flags (-O3 -ftree-vectorize -funroll-loops -ansi, then -std=c++11; no fast-math, no -march), into a temporary directory, against
the stand-in opencv2/ headers and the driver of tools/kaze_standin/, and driven through ctypes.  The stand-in header specifies the
OpenCV calls those sources make; the driver restates the few lines of the KAZE branch and reads the object's private members.
Per image case the fixture holds the keypoints after refinement, the raw maxima, the lists after the same-level / lower-level
pass and after the upper-level pass, the level table with every tau list, kcontrast, hmax and the histogram, per plane (Lt,
Lsmooth, Lflow, Ldet of every level) a SHA-256 digest and 64 seeded samples, and the whole planes of the two smallest cases; per
planted case the four lists.  Nothing of the reference and nothing compiled from it is written to the repository."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kaze_cases  # noqa: E402
import kaze_model as M  # noqa: E402

STANDIN = os.path.join(ROOT, "tools", "kaze_standin")
FLAGS = ["-O3", "-ftree-vectorize", "-funroll-loops", "-ansi", "-std=c++11", "-fPIC"]
PLANES = ("Lt", "Lsmooth", "Lflow", "Ldet")
MAX_LEVELS, MAX_TAU = 64, 256


def build(ref_root, tmp):
    cxx = os.environ.get("CXX", "c++")
    src = os.path.join(ref_root, "akaze", "src", "lib")
    so = os.path.join(tmp, "libkazeref.so")
    subprocess.check_call([cxx] + FLAGS + ["-shared", "-I" + STANDIN, "-I" + src] +
                          [os.path.join(src, f) for f in ("AKAZE.cpp", "nldiffusion_functions.cpp", "fed.cpp")] +
                          [os.path.join(STANDIN, "driver.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.kaze_new.restype = C.c_void_p
    lib.kaze_new.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]
    lib.kaze_free.argtypes = [C.c_void_p]
    lib.kaze_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.kaze_omax.argtypes = [C.c_void_p]
    lib.kaze_tau.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.kaze_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.kaze_plane.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.kaze_response.argtypes = [C.c_void_p]
    lib.kaze_plant.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.kaze_find.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


_p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


def _new(lib, rows, cols, par):
    return lib.kaze_new(rows, cols, par["omax"], par["nsublevels"], par["soffset"], par["derivative_factor"], par["dthreshold"],
                        par["min_dthreshold"], par["kcontrast_percentile"], par["kcontrast_nbins"], par["descriptor"])


def _levels(lib, h):
    table, sig = np.zeros((MAX_LEVELS, 6), np.int32), np.zeros((MAX_LEVELS, 2), np.float32)
    n = lib.kaze_levels(h, _p(table), _p(sig))
    tau = np.zeros((n, MAX_TAU), np.float32)
    for i in range(1, n):
        assert lib.kaze_tau(h, i, _p(tau[i])) == table[i, 5]
    return dict(levels=table[:n].copy(), sigmas=sig[:n].copy(), tau=tau[:, :max(1, int(table[:n, 5].max()))].copy(),
                omax=np.int32(lib.kaze_omax(h)))


def _kp(a):
    k = np.zeros(len(a), M.KP)
    for j, f in enumerate(("x", "y", "size", "response", "octave", "class_id")):
        k[f] = a[:, j]
    return k


def _find(lib, h, npx):
    cap = npx
    raw, rawv = np.zeros((cap, 3), np.int32), np.zeros(cap, np.float32)
    lists = [np.zeros((cap, 6), np.float64) for _ in range(3)]
    counts = np.zeros(4, np.int64)
    rc = lib.kaze_find(h, _p(raw), _p(rawv), cap, _p(lists[0]), _p(lists[1]), _p(lists[2]), cap, _p(counts))
    assert rc == 0, (rc, counts)
    n = [int(v) for v in counts]
    return dict(raw=raw[:n[0]].copy(), rawv=rawv[:n[0]].copy(), aux=_kp(lists[0][:n[1]]), upper=_kp(lists[1][:n[2]]),
                final=_kp(lists[2][:n[3]]))


def run(lib, img, par):
    """-> what the compiled reference computes for one image"""
    img = np.ascontiguousarray(img, np.float32)
    rows, cols = img.shape
    h = _new(lib, rows, cols, par)
    out = _levels(lib, h)
    kc, hist = np.zeros(3, np.float32), np.zeros(par["kcontrast_nbins"], np.int64)
    assert lib.kaze_create(h, _p(img), _p(kc), _p(hist)) == 0
    lib.kaze_response(h)
    out.update(kcontrast=kc[0], hmax=kc[1], kcontrast_last=kc[2], hist=hist)
    for w, name in enumerate(PLANES):
        planes = []
        for i, L in enumerate(out["levels"]):
            a = np.zeros((L[2], L[3]), np.float32)
            rc = lib.kaze_plane(h, i, w, _p(a))
            assert rc == 0 or (name == "Lflow" and i == 0) or (name == "Lsmooth"), (name, i)
            planes.append(a)
        out[name] = planes
    out.update(_find(lib, h, rows * cols))
    lib.kaze_free(h)
    return out


def run_planted(lib, name):
    (w, hh), par, _ = kaze_cases.PLANTED[name]
    _, _, planes = kaze_cases.planted(name)
    h = _new(lib, hh, w, par)
    for i, a in enumerate(planes):
        lib.kaze_plant(h, i, _p(np.ascontiguousarray(a)))
    out = _find(lib, h, w * hh)
    lib.kaze_free(h)
    return out


def main(ref_root, out):
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref_root, tmp)
        names = kaze_cases.names()
        data = dict(names=np.array(names), planted=np.array(sorted(kaze_cases.PLANTED)))
        for k, (name, img, par) in enumerate(kaze_cases.cases()):
            ref = run(lib, img, par)
            pre = "c%02d_" % k
            for key in ("levels", "sigmas", "tau", "omax", "kcontrast", "hmax", "kcontrast_last", "hist", "raw", "rawv", "aux", "upper", "final"):
                data[pre + key] = ref[key]
            flat = [a for nm in PLANES for a in ref[nm]]
            data[pre + "digests"] = np.stack([M.digest(a) for a in flat])
            data[pre + "samples"] = np.stack([a.reshape(-1)[M.sample_index(a.size)] for a in flat])
            if name in kaze_cases.WHOLE_PLANES:
                for nm in PLANES:
                    for i, a in enumerate(ref[nm]):
                        data[pre + "%s_%d" % (nm, i)] = a
            print("%-18s levels %2d k %.6f raw %5d aux %5d upper %5d final %5d" %
                  (name, len(ref["levels"]), ref["kcontrast"], len(ref["raw"]), len(ref["aux"]), len(ref["upper"]), len(ref["final"])))
        for name in sorted(kaze_cases.PLANTED):
            ref = run_planted(lib, name)
            for key, v in ref.items():
                data["p_%s_%s" % (name, key)] = v
            print("%-18s raw %5d aux %5d upper %5d final %5d" % (name, len(ref["raw"]), len(ref["aux"]), len(ref["upper"]), len(ref["final"])))
    np.savez_compressed(out, **data)
    print("cases", len(names), "->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
