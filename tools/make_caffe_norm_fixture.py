#!/usr/bin/env python3
"""Records what the reference's L2normalize / L1normalize / RootNormalize compute on the rows of tests/caffe_cases.py:
tests/golden/caffe_norm_ref.npz, the golden data of tests/test_caffe_model_cpu.py.  Run on a development machine that has the
reference's sources; needs a C++ compiler, no GPU:
    python tools/make_caffe_norm_fixture.py <reference root> tests/golden/caffe_norm_ref.npz
The three functions are found in imagerepresentation.cpp by their signatures and written, with a small main, into a temporary
directory; they are compiled there with the host compiler at -O2 -ffp-contract=off and fed the case rows through files.  Nothing
of the reference and nothing compiled from it is written to the repository: the fixture holds the rows and the recorded numbers."""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import caffe_cases  # noqa: E402

FUNCTIONS = ("L2normalize", "L1normalize", "RootNormalize")
SIGNATURE = "void %s(const float* input_arr, int size, std::vector<float> &output_vect)"
FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++14"]
MAIN = r"""
int main(int argc, char **argv) {
  int which = atoi(argv[1]), n = atoi(argv[2]), dim = atoi(argv[3]);
  std::vector<float> in((size_t)n * dim), out(dim);
  FILE *f = fopen(argv[4], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) return 2;
  fclose(f);
  f = fopen(argv[5], "wb");
  for (int i = 0; i < n; i++) {
    if (which == 0) L2normalize(in.data() + (size_t)i * dim, dim, out);
    else if (which == 1) L1normalize(in.data() + (size_t)i * dim, dim, out);
    else RootNormalize(in.data() + (size_t)i * dim, dim, out);
    if (fwrite(out.data(), 4, dim, f) != (size_t)dim) return 3;
  }
  return fclose(f) ? 4 : 0;
}
"""


def function_text(src, name):
    """the definition of `name`: from its signature to the brace that closes its body"""
    at = src.index(SIGNATURE % name)
    depth, i = 0, src.index("{", at)
    while True:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
        if depth == 0:
            return src[at:i]


def main(ref_root, out):
    src = open(os.path.join(ref_root, "imagerepresentation.cpp"), errors="replace").read()
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "norms.cpp"), os.path.join(tmp, "norms")
        with open(cpp, "w") as f:
            f.write("#include <math.h>\n#include <stdio.h>\n#include <stdlib.h>\n#include <vector>\n")
            f.write("\n".join(function_text(src, name) for name in FUNCTIONS))
            f.write(MAIN)
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + [cpp, "-o", exe, "-lm"])
        data = {}
        for w in caffe_cases.NORM_WIDTHS:
            rows = np.ascontiguousarray(caffe_cases.norm_rows(w), np.float32)
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            rows.tofile(fin)
            data["in_%d" % w] = rows
            for norm in caffe_cases.NORMS:
                subprocess.check_call([exe, str(norm), str(len(rows)), str(w), fin, fout])
                data["%s_%d" % (caffe_cases.NORM_NAMES[norm], w)] = np.fromfile(fout, np.float32).reshape(rows.shape)
    np.savez_compressed(out, **data)
    print("%s: %d arrays, %d bytes" % (out, len(data), os.path.getsize(out)))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
