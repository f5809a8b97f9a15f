"""CPU: the host side of the f32 FGINN matcher (mods_amd/csrc/fginn_walk.hpp: the open, close and emit steps that the single call
and the grouped call of the stored float classes both run) on its own.

tests/fginn_walk_main.cpp includes the header and the standard library only.  It is built with the host C++ compiler twice, plain
and with -fsanitize=address,undefined, and each binary runs as a child process under a time limit.  Nothing is loaded into this
process.  The program takes sorted neighbour lists as keys, plays the resolve sweep on the host from the kernel's definition and
prints records and stages; they are compared with the model the project already has, FC.walk (matching.cpp:385-457 restated) and
FC.expected_stage of tests/fginn32_cases.py: indices, the f32 distances and the f64 ratio bit for bit.

Inputs: the neighbour lists of FC.walk_case, short_case, tiny_case and threshold_case through FC.knn_f32_left_to_right at nn in
{2, 3, 4, 5, 50, 256} (the planted walks also at 7, 48 and 49: a record at rank nn - 1 exactly); random rows against n2 = 1 .. 5 trains; hand-made lists with d0 = 0 against d = 0 and against d > 0; and one
run of two problems (pad 0 and 1, different n2 and pos2) through one open list, whose outputs must equal those of each problem run
alone.  test_inputs_reach_every_end asserts from the model's own ends that these inputs reach a record and a contradiction on
both sides of j = 3, "nn reached", "trains ran out" and stage 2."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fginn32_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fginn_walk_main.cpp")
HEADER = os.path.join(ROOT, "mods_amd", "csrc", "fginn_walk.hpp")
LIMIT_S = 60             # either binary takes well under a second
BUILDS = {"plain": ["-O2"], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"]}
NNS = (2, 3, 4, 5, 50, 256)
WALK_NNS = (7, 48, 49)   # the planted records behind j = 3 at rank nn - 1 exactly (j = 6, j = 48) and one above it (stage 2)


def _problem(idx, dist, pos):
    """a problem of the case file from its FULL sorted neighbour list idx / dist [n1][n2] and pos [n2][2]"""
    return dict(idx=np.asarray(idx, np.int32), dist=np.asarray(dist, np.float32), pos=np.asarray(pos, np.float64))


def _from_case(c):
    idx, dist = FC.knn_f32_left_to_right(c["q"], c["t"], len(c["t"]))
    return _problem(idx, dist, c["pos"]), c["ratio"], c["cd"]


def _zero_lists():
    """hand-made lists (ties in index order): d0 = 0 against d = 0 -- 0 / 0 is NaN and fails -- until the far train 4 contradicts at
    j = 4, or until d = 1 passes at j = 2; d0 = 0 against d > 0: ratio 0 passes at j = 1; and nothing but zeros"""
    idx = np.array([[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [2, 0, 1, 3, 4, 5], [0, 1, 2, 3, 4, 5]], np.int32)
    dist = np.array([[0, 0, 0, 0, 0, 2], [0, 0, 1, 1, 1, 1], [0, 3, 3, 3, 3, 3], [0, 0, 0, 0, 0, 0]], np.float32)
    pos = np.array([[0, 0], [1, 0], [2, 0], [FC.CD, 0], [100, 0], [5, 0]], np.float64)      # train 3: exactly contradDist from train 0, no contradiction
    return _problem(idx, dist, pos)


def _two_problems():
    """the planted walks twice: another interleaving of the trains (other indices, other pos2) with the last seven trains left out"""
    a, ratio, cd = _from_case(FC.walk_case())
    c = FC.walk_case(seed=11)
    c["t"], c["pos"] = c["t"][:-7], c["pos"][:-7] + 3.0
    b, _, _ = _from_case(c)
    assert a["idx"].shape[0] == b["idx"].shape[0] and a["idx"].shape[1] != b["idx"].shape[1]
    return a, b, ratio, cd


@pytest.fixture(scope="module")
def runs():
    """every run of the case file: (name, problems, nn, ratio, cd)"""
    out = []
    for name, case in (("walk", FC.walk_case()), ("short", FC.short_case()), ("tiny", FC.tiny_case()), ("threshold", FC.threshold_case())):
        p, ratio, cd = _from_case(case)
        out += [("%s_nn%d" % (name, nn), [p], nn, ratio, cd) for nn in NNS + (WALK_NNS if name == "walk" else ())]
    for n2 in (1, 2, 3, 4, 5):
        p, ratio, cd = _from_case(FC.random_case(9, n2, 8, 20 + n2))
        out += [("n2_%d_nn%d" % (n2, nn), [p], nn, ratio, cd) for nn in (2, 4, 5, 50)]
    out += [("zero_nn%d" % nn, [_zero_lists()], nn, FC.RATIO, FC.CD) for nn in (2, 4, 6, 50)]
    a, b, ratio, cd = _two_problems()
    out += [("pair_a", [a], 50, ratio, cd), ("pair_b", [b], 50, ratio, cd), ("pair_ab", [a, b], 50, ratio, cd)]
    return out


def _model(p, nn, ratio, cd):
    tents, ends = FC.walk(p["idx"], p["dist"], p["pos"], ratio, cd, nn)
    return tents, ends, FC.expected_stage(p["idx"], p["dist"], p["pos"], ratio, cd, nn)


def _f64_bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def _case_file(runs, path):
    with open(path, "w") as f:
        for _, probs, nn, ratio, cd in runs:
            f.write("%x %x %x %x %x\n" % (len(probs), probs[0]["idx"].shape[0], nn, _f64_bits(ratio), _f64_bits(cd)))
            for p in probs:
                n1, n2 = p["idx"].shape
                keys = (p["dist"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | p["idx"].astype(np.uint64)
                assert np.all(keys[:, 1:] > keys[:, :-1]), "the lists are sorted by key"
                f.write("%x\n" % n2)
                f.write(" ".join("%x" % v for v in p["pos"].reshape(-1).view(np.uint64)) + "\n")
                for q in range(n1):
                    f.write(" ".join("%x" % int(k) for k in keys[q]) + "\n")


def _parse(text):
    """[[(records, stages) per problem] per run]"""
    out, lines, i = [], text.split("\n"), 0
    while i < len(lines) and lines[i].startswith("run "):
        np_ = int(lines[i].split()[1])
        i += 1
        probs = []
        for p in range(np_):
            head = lines[i].split()
            assert head[0] == "problem" and int(head[1]) == p, lines[i]
            recs = [tuple(int(w) for w in ln.split()[:4]) + tuple(int(w, 16) for w in ln.split()[4:]) for ln in lines[i + 1:i + 1 + int(head[2])]]
            i += 1 + int(head[2])
            assert lines[i].startswith("stages "), lines[i]
            probs.append((recs, [int(ch) for ch in lines[i].split()[1]] if len(lines[i].split()) > 1 else []))
            i += 1
        out.append(probs)
    assert i == len(lines) - 1 and lines[i] == "", lines[i:i + 3]
    return out


@pytest.fixture(scope="module")
def cxx():
    for name in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    pytest.fail("no host C++ compiler (g++, c++, clang++) to build tests/fginn_walk_main.cpp with")


def test_header_is_host_only():
    """plain C++17: the standard library and modsx.h, nothing of HIP or of the engine"""
    text = open(HEADER).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all((i.startswith("<") and "hip" not in i) or i == '"../../include/modsx.h"' for i in includes), includes
    main = [ln.split()[1] for ln in open(SRC).read().splitlines() if ln.startswith("#include")]
    assert all(i.startswith("<") or i == '"../mods_amd/csrc/fginn_walk.hpp"' for i in main), main


def test_inputs_reach_every_end(runs):
    reached, stages = set(), set()
    for _, probs, nn, ratio, cd in runs:
        for p in probs:
            _, ends, stage = _model(p, nn, ratio, cd)
            reached |= {(what, "j<=3" if j <= 3 else "j>3") for what, j in ends if what in ("record", "contradiction")}
            reached |= {what for what, _ in ends if what in ("nn", "trains")}
            stages |= set(int(s) for s in stage)
    assert reached >= {("record", "j<=3"), ("record", "j>3"), ("contradiction", "j<=3"), ("contradiction", "j>3"), "nn", "trains"}, reached
    assert stages == {0, 1, 2}, stages
    # d0 = 0 against d = 0 and against d > 0, in the hand-made lists
    z = _zero_lists()
    assert z["dist"][0, 0] == 0 and z["dist"][0, 1] == 0 and z["dist"][2, 0] == 0 and z["dist"][2, 1] > 0


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_walk_program_matches_the_model(cxx, tmp_path, runs, build):
    exe, cases = str(tmp_path / ("fginn_walk_" + build)), str(tmp_path / "cases.txt")
    subprocess.run([cxx, "-std=c++17", "-Wall"] + BUILDS[build] + [SRC, "-o", exe], check=True, timeout=300)
    _case_file(runs, cases)
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=LIMIT_S)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stdout[-1000:], out.stderr[-4000:])
    got = _parse(out.stdout)
    assert len(got) == len(runs)
    for (name, probs, nn, ratio, cd), res in zip(runs, got):
        assert len(res) == len(probs), name
        for p, (recs, stage) in zip(probs, res):
            tents, _, want_stage = _model(p, nn, ratio, cd)
            want = [t[:4] + tuple(_f64_bits(v) for v in t[4:]) for t in tents]
            assert recs == want, (name, len(recs), len(want))
            assert stage == [int(s) for s in want_stage], name
    # two problems through one open list: each problem's output is its output run alone
    by_name = {r[0]: g for r, g in zip(runs, got)}
    assert by_name["pair_ab"] == [by_name["pair_a"][0], by_name["pair_b"][0]]
    assert by_name["pair_a"][0] != by_name["pair_b"][0] and by_name["pair_a"][0][0] and by_name["pair_b"][0][0]
