#!/usr/bin/env python3
"""Records what the reference's libdaisy computes on the patches of tests/daisy_cases.py: tests/golden/daisy_ref.npz, the golden
data of tests/test_daisy_model_cpu.py.  Run on a development machine that has the reference's sources and the built oracle (the
region patches of the case list come from it); needs a C++ compiler, no GPU and no OpenCV:
    python tools/make_daisy_fixture.py <reference root> tests/golden/daisy_ref.npz
The reference's libdaisy/src/daisy.cpp, general.cpp and interaction.cpp are compiled as they are, with the reference's own flags
(-O3 -ftree-vectorize -funroll-loops -ansi, then -std=c++11; no fast-math, no -march), into a temporary directory, together with
the driver of tools/daisy_standin/, and driven through ctypes.  The driver restates the byte conversion and the few lines of
descriptors/daisydescriptor.hpp.  The fixture holds, per parameter set and normalisation, the row of every case patch; per
parameter set the grid, the selected cubes, the filter taps (kutility::gaussian_1d at the lengths and sigmas of the model's
tables, whose rows pin them) and one layer of every cube of one patch; and the blurred image, dx and dy of a few patches.
Nothing of the reference and nothing compiled from it is written to the repository.  The tool also prints the libm functions the
compiled daisy.cpp imports (expf, sincos, sqrt, sqrtf here): the library's host tables and the model call the same ones."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import daisy_cases  # noqa: E402
import daisy_model as M  # noqa: E402

STANDIN = os.path.join(ROOT, "tools", "daisy_standin")
FLAGS = ["-w", "-O3", "-ftree-vectorize", "-funroll-loops", "-ansi", "-std=c++11", "-fPIC"]
LIBM = ("exp", "sin", "cos", "sqrt", "atan", "pow", "log", "fabs", "floor", "ceil", "rint", "nearbyint", "round")


def main(ref_root, out):
    cxx = os.environ.get("CXX", "c++")
    daisy = os.path.join(ref_root, "libdaisy")
    inc = ["-I" + os.path.join(daisy, "include"), "-I" + os.path.join(daisy, "include", "kutility")]
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        for name in ("daisy", "general", "interaction"):
            objs.append(os.path.join(tmp, name + ".o"))
            subprocess.check_call([cxx] + FLAGS + inc + ["-c", os.path.join(daisy, "src", name + ".cpp"), "-o", objs[-1]])
        syms = subprocess.check_output(["nm", "-u", objs[0]]).decode().split()
        print("daisy.o imports:", sorted(s for s in syms if s.startswith(LIBM) and len(s) < 12))
        so = os.path.join(tmp, "libdaisyref.so")
        subprocess.check_call([cxx] + FLAGS + ["-shared"] + inc + objs + [os.path.join(STANDIN, "driver.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.daisy_ref.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p]
        lib.daisy_grad.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.daisy_consts.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        names = daisy_cases.names()
        pats = np.ascontiguousarray(daisy_cases.patches(), np.float32)
        planes_of = [names.index(n) for n in daisy_cases.PLANES_OF]
        cubes_of = names.index(daisy_cases.CUBES_OF)
        data = dict(names=np.array(names), params=np.array(daisy_cases.PARAMS, np.int32), planes_of=np.array(planes_of, np.int32),
                    cubes_of=np.int32(cubes_of), cube_layer=np.int32(daisy_cases.CUBE_LAYER))
        planes = np.zeros((len(planes_of), 3, 41, 41), np.float32)
        for i, k in enumerate(planes_of):
            lib.daisy_grad(p(pats[k]), 41, p(planes[i, 0]), p(planes[i, 1]), p(planes[i, 2]))
        data["planes"] = planes
        k5 = np.zeros(5, np.float32)
        lib.daisy_consts(41, 0, 0, 0, 0, None, None, 5, C.c_float(0.5), p(k5))
        data["k5"] = k5
        for s, (rad, radq, thq, histq) in enumerate(daisy_cases.PARAMS):
            dim = M.dim(radq, thq, histq)
            for nrm in daisy_cases.NRMS:
                rows = np.full((len(pats), dim), np.nan, np.float32)
                for i in range(len(pats)):
                    cubes = np.zeros((radq, 41, 41), np.float32)
                    got = lib.daisy_ref(p(pats[i]), 41, rad, radq, thq, histq, nrm, p(rows[i]), daisy_cases.CUBE_LAYER,
                                        p(cubes) if i == cubes_of else None)
                    assert got == dim
                    if i == cubes_of:
                        data["cubes_%d" % s] = cubes[:, :40, :40].copy()     # compute_histograms leaves row and column 40 unwritten
                data["desc_%d_%d" % (s, nrm)] = rows
            grid, sel = np.zeros((radq * thq + 1, 2), np.float64), np.zeros(radq, np.int32)
            lib.daisy_consts(41, rad, radq, thq, histq, p(grid), p(sel), 0, C.c_float(0), None)
            T = M.tables(rad, radq, thq, histq)
            taps = np.zeros((1 + radq, M.MAX_TAPS), np.float32)
            for f in range(1 + radq):
                lib.daisy_consts(41, 0, 0, 0, 0, None, None, int(T["fsz"][f]), C.c_float(T["sigmas"][f]), p(taps[f]))
            data.update({"grid_%d" % s: grid, "selected_%d" % s: sel, "taps_%d" % s: taps})
    np.savez_compressed(out, **data)
    print("patches", len(names), "parameter sets", len(daisy_cases.PARAMS), "->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
