"""CPU: the thread logic of the batch calls (mods_amd/csrc/batch_driver.hpp) on its own.

tests/batch_driver_main.cpp includes the header and the standard library only.  It is built with the host C++ compiler twice, plain
and with -fsanitize=thread, and each binary runs as a child process under a time limit: a deadlock shows as a timeout, a data race
as ThreadSanitizer's report and exit code.  Nothing is loaded into this process.

What the program asserts, over the shapes (n_ctx, n, group_cap) = (1,0,4) (1,1,4) (3,1,4) (2,5,4) (2,9,4) (4,3,1) (3,7,1), helpers
of 1 and of nw, producers that emit zero, one and `count` tasks per group: every item is produced once and every pushed task is
consumed once; nothing runs after the call has returned; worker 0 is the caller's thread and at most nw worker threads are seen; nw
and group are the formulas of the batch entries; with the failing item first, in the middle, last, and with two failures of
different codes the call returns one of the codes with that code's own text, consumes no task of a failed group and none twice."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "batch_driver_main.cpp")
REPS = 40                # runs per shape and failure set; about 6 000 batch runs in all
LIMIT_S = 120            # the plain binary takes about a second, the sanitizer's a few
BUILDS = {"plain": ["-O2"], "tsan": ["-fsanitize=thread", "-O1", "-g"]}


@pytest.fixture(scope="module")
def cxx():
    for name in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail("no host C++ compiler (g++, c++, clang++) to build tests/batch_driver_main.cpp with")


def test_header_is_host_only():
    """plain C++17: nothing of HIP, of the engine or of the C ABI is included"""
    text = open(os.path.join(ROOT, "mods_amd", "csrc", "batch_driver.hpp")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_batch_driver_program(cxx, tmp_path, build):
    exe = str(tmp_path / ("batch_driver_" + build))
    subprocess.run([cxx, "-std=c++17", "-Wall", "-pthread"] + BUILDS[build] + [SRC, "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe, str(REPS)], capture_output=True, text=True, timeout=LIMIT_S)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.startswith("batch driver ok") and "ThreadSanitizer" not in out.stderr, (out.stdout, out.stderr[-4000:])
