#!/usr/bin/env python3
"""Records what the reference's SIFT code computes on the inputs of tests/dspsift_cases.py: tests/golden/dspsift_ref.npz, the
golden data of tests/test_dspsift_model_cpu.py.  Run on a development machine that has the reference's sources and the built
oracle (the region patches of the case list come from it); needs a C++ compiler, no GPU and no OpenCV:
    python tools/make_dspsift_fixture.py <reference root> tests/golden/dspsift_ref.npz
The reference's matching/siftdesc.cpp and detectors/helpers.cpp are compiled as they are, with the reference's own flags (-O3
-ftree-vectorize -funroll-loops, no fast-math, no -march), into a temporary directory, against the stand-in OpenCV headers and
the driver of tools/dspsift_standin/, and driven through ctypes.  For every case patch the fixture holds the output of
SIFTDescriptor{useRootSIFT = false, doNorm = false}, for every case row SIFTnorm(std::vector<float>&) at maxBinValue 0.2 and at
(double)0.2f.  Nothing of the reference and nothing compiled from it is written to the repository."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dspsift_cases  # noqa: E402

STANDIN = os.path.join(ROOT, "tools", "dspsift_standin")
FLAGS = ["-O3", "-ftree-vectorize", "-funroll-loops", "-fPIC", "-shared"]


def main(ref_root, out):
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libdspsiftref.so")
        subprocess.check_call([os.environ.get("CXX", "c++")] + FLAGS +
                              ["-I" + STANDIN, "-I" + ref_root, "-I" + os.path.join(ref_root, "detectors"),
                               os.path.join(ref_root, "matching", "siftdesc.cpp"), os.path.join(ref_root, "detectors", "helpers.cpp"),
                               os.path.join(STANDIN, "driver.cpp"), "-o", so])
        lib = C.CDLL(so)
        lib.dsp_raw.argtypes = [C.c_void_p, C.c_void_p]
        lib.dsp_norm.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        raw = []
        for patch in dspsift_cases.patches():
            patch = np.ascontiguousarray(patch, np.float32)
            h = np.zeros(128, np.float32)
            lib.dsp_raw(p(patch), p(h))
            raw.append(h)
        norms = []
        for mb in dspsift_cases.MAX_BINS:
            rows = []
            for _, row in dspsift_cases.norm_rows():
                row = np.ascontiguousarray(row, np.float32)
                o = np.zeros(128, np.float32)
                lib.dsp_norm(p(row), C.c_double(mb), p(o))
                rows.append(o)
            norms.append(np.stack(rows))
    # the outputs are integers 0..255: bytes hold them
    norms = np.stack(norms)
    assert (norms == norms.astype(np.uint8)).all()
    np.savez_compressed(out, patch_names=np.array(dspsift_cases.patch_names()), raw=np.stack(raw),
                        row_names=np.array([n for n, _ in dspsift_cases.norm_rows()]), max_bins=np.array(dspsift_cases.MAX_BINS, np.float64),
                        norm=norms.astype(np.uint8))
    print("patches", len(raw), "rows", norms.shape[1], "->", out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
