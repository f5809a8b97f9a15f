#!/usr/bin/env python3
"""Records what the reference's OpenSURF code computes on the patches of tests/surf_cases.py: tests/golden/surf_ref.npz, the
golden data of tests/test_surf_model_cpu.py.  Run on a development machine that has the reference's sources and the built oracle
(the region patches of the case list come from it); needs a C++ compiler, no GPU and no OpenCV:
    python tools/make_surf_fixture.py <reference root> tests/golden/surf_ref.npz
The reference's opensurf/surf.cpp and opensurf/integral.cpp are compiled as they are, with the reference's own flags (-O3
-ftree-vectorize -funroll-loops -ansi, then -std=c++11; no fast-math, no -march), into a temporary directory, against the
stand-in opencv/cv.h and the driver of tools/surf_standin/, and driven through ctypes.  The driver restates getGray and the few
lines of descriptors/surfdescriptor.hpp.  Per case mrSize the fixture holds the descriptor of every case patch, the integral
image of a few, and the coordinate and weight tables.  Nothing of the reference and nothing compiled from it is written to the
repository.  The tool also prints which exponential the compiled surf.cpp imports (expf here): the library's host tables and
the model call the same one."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import surf_cases  # noqa: E402

STANDIN = os.path.join(ROOT, "tools", "surf_standin")
FLAGS = ["-O3", "-ftree-vectorize", "-funroll-loops", "-ansi", "-std=c++11", "-fPIC"]


def main(ref_root, out):
    cxx = os.environ.get("CXX", "c++")
    inc = ["-I" + STANDIN, "-I" + os.path.join(ref_root, "opensurf")]
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "surf.o")
        subprocess.check_call([cxx] + FLAGS + inc + ["-c", os.path.join(ref_root, "opensurf", "surf.cpp"), "-o", obj])
        syms = subprocess.check_output(["nm", "-u", obj]).decode().split()
        print("surf.o imports:", sorted(s for s in syms if s.startswith("exp")))
        so = os.path.join(tmp, "libsurfref.so")
        subprocess.check_call([cxx] + FLAGS + ["-shared"] + inc +
                              [obj, os.path.join(ref_root, "opensurf", "integral.cpp"), os.path.join(STANDIN, "driver.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.surf_ref.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        lib.surf_tables.argtypes = [C.c_int, C.c_double] + [C.c_void_p] * 5
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        names = surf_cases.names()
        which = [names.index(n) for n in surf_cases.INTEGRAL_OF]
        assert which == sorted(which)
        data = dict(names=np.array(names), mr_sizes=np.array(surf_cases.MR_SIZES, np.float64), integral_of=np.array(which, np.int32))
        for m, mr in enumerate(surf_cases.MR_SIZES):
            descs, ints = [], []
            for i, patch in enumerate(surf_cases.patches()):
                patch = np.ascontiguousarray(patch, np.float32)
                d, ii = np.zeros(64, np.float32), np.zeros((41, 41), np.float32)
                lib.surf_ref(p(patch), 41, C.c_double(mr), p(d), p(ii))
                descs.append(d)
                if i in which:
                    ints.append(ii)
            sx, sy = np.zeros(24, np.int32), np.zeros(24, np.int32)
            w1, w2, hs = np.zeros((16, 81), np.float32), np.zeros(16, np.float32), np.zeros(1, np.int32)
            lib.surf_tables(41, C.c_double(mr), p(sx), p(sy), p(w1), p(w2), p(hs))
            data.update({"desc_%d" % m: np.stack(descs), "integral_%d" % m: np.stack(ints), "sample_x_%d" % m: sx,
                         "sample_y_%d" % m: sy, "w1_%d" % m: w1, "w2_%d" % m: w2, "haar_size_%d" % m: hs})
    np.savez_compressed(out, **data)
    print("patches", len(names), "mrSize values", len(surf_cases.MR_SIZES), "->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
