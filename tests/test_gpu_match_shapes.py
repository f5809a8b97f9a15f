"""GPU: the FGINN matcher against the oracle in every shape of k_match_sweep1<QS, FAT> / k_match_resolve<QS>, across index-chunk
boundaries and at the big sizes (cases and their coverage proofs: tests/match_cases.py, tests/test_match_cases_cpu.py).

Default shape, in this process: the chunk cases and the big cases through the session's context; after every call
mods_amd.last_match_geometry() must report what the restated layout predicts -- the only place where the Python restatement and
the launcher meet.  A mismatch there means the restatement is wrong, and the coverage proofs with it: fix the restatement.

Forced shapes: MODSX_MATCH_QSETS and MODSX_SWEEP1_FAT are read once per process, so every shape gets ONE fresh child
(tests/match_shape_child.py) that runs the whole table on one context and the ten-pair batch of test_grouped_pairs_equal_single_pairs;
the parent compares what comes back with references it computed once.  Every field of every tentative must be equal.

Fault latch: a child that ends by a signal, with status 134 / 139, by the time limit, or with any failure whose stderr carries a HIP
error sets _FAULT; every later test of this module then
fails at once with that child's stderr tail -- no further process, no further use of the context, no retry."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import match_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "match_shape_child.py")
GEO = ("qs", "fat", "S", "tiles_per_split", "ntiles_ub")
# Time limit of a child.  Measured on an MI355X: the slowest child (<2,fat>: the whole table, 57 calls, and the ten-pair batch) took
# 0.8 s from start to exit; five times that, rounded up to a multiple of 30 s, is 30 s, and the floor of 120 s applies (import,
# context creation and a shared GPU vary by that much).
CHILD_TIMEOUT_S = 120
_FAULT = None          # (what happened, stderr tail) of the first child that faulted or hung


def _latch():
    if _FAULT is not None:
        pytest.fail("an earlier matcher child %s; nothing more is started on the GPU.  Its stderr ended:\n%s" % _FAULT, pytrace=False)


def _all_cases(which):
    return {"all": MC.small_cases() + MC.chunk_cases() + MC.big_cases(), "chunk": MC.chunk_cases()}[which]


@pytest.fixture(scope="module")
def refs(oracle):
    """oracle tentatives of every (case, parameter set), computed once and left alone"""
    out = {}
    for c in _all_cases("all"):
        for pi, p in enumerate(c.params):
            r = oracle.match_fginn(c.d1, c.d2, c.pos2, *p)
            r.setflags(write=False)
            out[c.name, pi] = r
    return out


def _same(got, ref, case, pi, shape, tmp_path):
    """every field equal (NaN == NaN: the ratio of 0 / 0); a case that differs is kept as .npz for reduction"""
    bad = None
    if len(got) != len(ref):
        bad = "%d tentatives against the oracle's %d" % (len(got), len(ref))
    else:
        for f in ref.dtype.names:
            if not np.array_equal(got[f], ref[f], equal_nan=ref[f].dtype.kind == "f"):
                bad = "field %s differs at tentative %d" % (f, int(np.nonzero(~((got[f] == ref[f]) | ((got[f] != got[f]) & (ref[f] != ref[f]))))[0][0]))
                break
    if bad:
        ratio, cd, nn = case.params[pi]
        path = os.path.join(str(tmp_path), "mismatch_%s_%d.npz" % (case.name, pi))
        np.savez(path, d1=case.d1.astype(np.uint8), d2=case.d2.astype(np.uint8), pos2=case.pos2, ratio=ratio, cd=cd, nn=nn, got=got, ref=ref)
        pytest.fail("%s %r under shape %r: %s (inputs and both results: %s)" % (case.name, case.params[pi], shape, bad, path), pytrace=False)


def _check_geo(geo, case, shape, what):
    lay = MC.layout(len(case.d1), len(case.d2), *shape)
    want = tuple(lay[k] for k in GEO)
    assert tuple(int(v) for v in geo) == want, "%s %s: the launcher used %r, the restated layout says %r (%r)" % (case.name, what, tuple(geo), want, GEO)


# ---------------- the default shape, in process ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.chunk_cases() + MC.big_cases(), ids=lambda c: c.name)
def test_default_shape_equals_oracle(ctx, modsx, refs, case, tmp_path):
    _latch()
    assert not os.environ.get("MODSX_MATCH_QSETS") and not os.environ.get("MODSX_SWEEP1_FAT"), "this test is about the sizes the launcher picks"
    shape = MC.default_shape(len(case.d1), len(case.d2))
    for pi, p in enumerate(case.params):
        got = ctx.match_fginn(case.d1, case.d2, case.pos2, *p)
        g = modsx.last_match_geometry()
        _check_geo([g[k] for k in GEO], case, shape, "in process")
        _same(got, refs[case.name, pi], case, pi, shape, tmp_path)
    assert max(len(refs[case.name, pi]) for pi in range(len(case.params))) >= 5, "nothing was compared"
    print("default shape %r: %s, %d tentatives compared" % (shape, case.name, sum(len(refs[case.name, pi]) for pi in range(len(case.params)))))


# ---------------- forced shapes, one child each -----------------------------------------------------------------------------------
HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "device-side assert",
                   "unspecified launch failure", "queue error")


def _run_child(cases, shape, pair, tmp_path):
    global _FAULT
    inp, outp = os.path.join(str(tmp_path), "in.npz"), os.path.join(str(tmp_path), "out.npz")
    z = dict(names=np.array([c.name for c in cases]), batch=np.array(int(pair is not None)))
    if pair is not None:
        z["pair_a"], z["pair_b"] = pair
    for i, c in enumerate(cases):
        z["d1_%d" % i], z["d2_%d" % i] = c.d1.astype(np.uint8), c.d2.astype(np.uint8)
        z["pos2_%d" % i], z["params_%d" % i] = c.pos2, np.array(c.params, np.float64)
    np.savez(inp, **z)
    env = dict(os.environ, MODSX_MATCH_QSETS=str(shape[0]), MODSX_SWEEP1_FAT=str(shape[1]))
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, CHILD, inp, outp], env=env, timeout=CHILD_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except subprocess.TimeoutExpired as e:
        _FAULT = ("for shape %r did not end within %d s" % (shape, CHILD_TIMEOUT_S), (e.stderr or b"").decode(errors="replace")[-1500:])
        _latch()
    err = p.stderr.decode(errors="replace")[-1500:]
    whole = p.stderr.decode(errors="replace").lower()
    if p.returncode < 0 or p.returncode in (134, 139) or (p.returncode != 0 and any(m in whole for m in HIP_ERROR_MARKS)):
        # (a fault that HIP reports as an error code reaches Python as a RuntimeError and status 1: the card is no better for it)
        _FAULT = ("for shape %r ended with status %d" % (shape, p.returncode), err)
        _latch()
    assert p.returncode == 0, "the child for shape %r failed with status %d:\n%s" % (shape, p.returncode, err)
    return np.load(outp), time.time() - t0


def _check_child(out, cases, shape, refs, tmp_path):
    n = 0
    for i, c in enumerate(cases):
        for pi in range(len(c.params)):
            geo = out["geo_%d_%d" % (i, pi)]
            assert (int(geo[0]), int(geo[1])) == shape, "%s: the forced shape %r was not taken: %r" % (c.name, shape, tuple(geo))
            _check_geo(geo, c, shape, "in the child")
            _same(out["tent_%d_%d" % (i, pi)], refs[c.name, pi], c, pi, shape, tmp_path)
            n += len(refs[c.name, pi])
    return n


def _check_batch(out, shape):
    """as test_gpu_parity.test_grouped_pairs_equal_single_pairs, on one context"""
    assert int(out["n_batch"]) == 10
    for i in range(10):
        for f in ("regions", "scalars", "verified", "H"):
            assert np.array_equal(out["batch_%d_%s" % (i, f)], out["single_%d_%s" % (i, f)]), (i, f)
        g, s = out["batch_%d_tentatives" % i], out["single_%d_tentatives" % i]
        assert len(g) == len(s), i
        for f in s.dtype.names:
            assert np.array_equal(g[f], s[f]), (i, f)
    assert sum(len(out["single_%d_tentatives" % i]) for i in range(10)) > 50
    for k in ("geo_single", "geo_batch"):
        assert (int(out[k][0]), int(out[k][1])) == shape, "%s: the batch did not run with the forced shape %r: %r" % (k, shape, tuple(out[k]))


@pytest.mark.parametrize("shape,which", [((2, 1), "all"), ((4, 0), "all"), ((4, 1), "all"), ((2, 0), "chunk")],
                         ids=["qs2_fat", "qs4_thin", "qs4_fat", "qs2_thin_chunk_cases"])
def test_forced_shape_equals_oracle(refs, small_pair, tmp_path, shape, which):
    _latch()
    cases = _all_cases(which)
    out, wall = _run_child(cases, shape, small_pair[:2] if which == "all" else None, tmp_path)
    n = _check_child(out, cases, shape, refs, tmp_path)
    if which == "all":
        _check_batch(out, shape)
    print("forced shape %r: %d cases, %d calls, %d oracle tentatives compared; child %.1f s (context %.1f s, cases %.1f s, in all %.1f s)"
          % (shape, len(cases), sum(len(c.params) for c in cases), n, wall, float(out["t_context"]), float(out["case_seconds"].sum()),
             float(out["t_total"])))
