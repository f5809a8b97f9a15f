#!/usr/bin/env python3
"""Records what the reference's LIOP code computes on the patches of tests/liop_cases.py: tests/golden/liop_ref.npz, the golden
data of tests/test_liop_model_cpu.py.  Run on a development machine that has the reference's sources; needs a C compiler, no GPU:
    python tools/make_liop_fixture.py <reference root> tests/golden/liop_ref.npz
VLFeat's liop.c, generic.c, host.c, random.c and mathop.c are compiled as they are into a temporary directory (no threads, no
SSE2 / AVX paths, no -march, no fast-math, no contraction) and driven through ctypes.  Nothing of the reference and nothing compiled
from it is written to the repository: the fixture holds descriptors, the sample tables and the sorted permutations only."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import liop_cases  # noqa: E402

SOURCES = ("liop.c", "generic.c", "host.c", "random.c", "mathop.c")
FLAGS = ["-O2", "-fPIC", "-shared", "-DVL_DISABLE_THREADS", "-DVL_DISABLE_SSE2", "-DVL_DISABLE_AVX", "-ffp-contract=off",
         "-fno-fast-math"]


class VlLiopDesc(C.Structure):      # vl/liop.h:22-44 (vl_int = int, vl_size = vl_uindex = 64-bit)
    _fields_ = [("numNeighbours", C.c_int), ("numSpatialBins", C.c_int), ("intensityThreshold", C.c_float),
                ("dimension", C.c_uint64), ("patchSideLength", C.c_uint64), ("patchSize", C.c_uint64),
                ("patchPixels", C.POINTER(C.c_uint64)), ("patchIntensities", C.POINTER(C.c_float)),
                ("patchPermutation", C.POINTER(C.c_uint64)), ("neighRadius", C.c_float),
                ("neighIntensities", C.POINTER(C.c_float)), ("neighPermutation", C.POINTER(C.c_uint64)),
                ("neighSamplesX", C.POINTER(C.c_double)), ("neighSamplesY", C.POINTER(C.c_double))]


def main(ref_root, out):
    vl = os.path.join(ref_root, "vlfeat", "vl")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libliopref.so")
        subprocess.check_call([os.environ.get("CC", "cc")] + FLAGS + ["-I" + os.path.join(ref_root, "vlfeat")] +
                              [os.path.join(vl, s) for s in SOURCES] + ["-o", so, "-lm"])
        lib = C.CDLL(so)
        lib.vl_liopdesc_new_basic.restype = C.POINTER(VlLiopDesc)
        lib.vl_liopdesc_new_basic.argtypes = [C.c_uint64]
        lib.vl_liopdesc_process.argtypes = [C.POINTER(VlLiopDesc), C.c_void_p, C.c_void_p]
        lib.vl_liopdesc_delete.argtypes = [C.POINTER(VlLiopDesc)]
        d = lib.vl_liopdesc_new_basic(41)
        s = d.contents
        n = int(s.patchSize)
        assert (s.numNeighbours, s.numSpatialBins, int(s.dimension), int(s.patchSideLength)) == (4, 6, 144, 41)
        pixels = np.array([s.patchPixels[i] for i in range(n)], np.int64)
        sx = np.array([s.neighSamplesX[i] for i in range(4 * n)], np.float64).reshape(n, 4)
        sy = np.array([s.neighSamplesY[i] for i in range(4 * n)], np.float64).reshape(n, 4)
        names, descs, perms = [], [], []
        for name, patch in liop_cases.cases():
            # two guard floats behind the patch: the sample of pixel (20, 34) reads them (times a weight of 0, liop.c:515-519)
            buf = np.zeros(41 * 41 + 2, np.float32)
            buf[:41 * 41] = patch.reshape(-1)
            desc = np.zeros(144, np.float32)
            lib.vl_liopdesc_process(d, desc.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p))
            names.append(name)
            descs.append(desc)
            perms.append(np.array([s.patchPermutation[i] for i in range(n)], np.uint16))
        thr = float(s.intensityThreshold)
        lib.vl_liopdesc_delete(d)
    np.savez_compressed(out, names=np.array(names), desc=np.stack(descs), perm=np.stack(perms), pixels=pixels, sx=sx, sy=sy,
                        intensity_threshold=np.float32(thr))
    print("patches", len(names), "measurement pixels", n, "->", out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
