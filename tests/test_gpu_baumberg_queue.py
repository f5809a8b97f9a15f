"""GPU: the queue-fed form of k_baumberg_stream (variant 3 of baumberg_geometry; mods_amd/csrc/kernels_affine.hip) against the oracle's
findAffineShape and against the static-chunk form (variant 0), keypoint by keypoint, through Context.debug_baumberg.

Comparison rule, everywhere: u[4], ok and iters of EVERY job are bit-equal to oracle.find_affine_shape_batch and to variant 0, failed
keypoints included; no job is left unwritten (the entry fills the result buffer with 0xFF bytes: iters == -1); the eight counters
handed out exactly n keypoints (each clipped to its range); and the geometry the launch reports is baumberg_geometry(n, 19, 3, chunk)
-- Context.baumberg_geometry, which knows the device the production rule (chunk 0) counts the resident wavefronts of; for a forced
chunk the host-only module function must give the same.

The jobs are those of tests/baumberg_cases.py on its five planes; tests/test_baumberg_queue_model_cpu.py shows on the CPU what the
refill rule does with them.
  1. whole list: production rule, 1 wavefront per range, 3, 8, and 400 per range (3 200 wavefronts for 1 295 jobs)
  2. prefixes n = 0, 1, 2, 7, 8, 9, 17 (fewer jobs than ranges, empty ranges), at the production rule, 1 and 3 per range
  3. the front-loaded list of the CPU test (every iteration-limit job in the first range), production rule, 1 and 8 per range
  4. maxIterations = 0 and 1, production rule and 1 per range
  5. production: detect_affine_keypoints in child processes with MODSX_BAUMBERG_QUEUE=0 and =1 returns the records of this process

Fault latch (test 5): a child that ends by a signal, with status 134 / 139, by its time limit, or with a HIP error on stderr makes
every later test of this module fail at once -- nothing more is started on the GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import baumberg_cases as BC
from tests import baumberg_queue_child as QC
from tests import baumberg_queue_model as QM
from tests.common import same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "baumberg_queue_child.py")
CHILD_TIMEOUT_S = 120      # import, context creation and four small detections: a second of work, the rest is what a shared machine may add
HIP_ERROR_MARKS = ("illegal memory access", "memory access fault", "hsa_status_error", "hiperror", "hip error", "device-side assert",
                   "unspecified launch failure", "queue error")
_FAULT = None


def _latch():
    if _FAULT is not None:
        pytest.fail("a child of this module %s; nothing more is started on the GPU.  Its stderr ended:\n%s" % _FAULT, pytrace=False)


@pytest.fixture(scope="module")
def dplanes(ctx, oracle):
    ims = [ctx.upload(p) for p in BC.planes(oracle)]     # f32, 1 channel: stored unchanged
    yield ims
    for im in ims:
        im.free()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref, what):
    n = len(ref["ok"])
    assert len(got["ok"]) == n
    unwritten = np.nonzero(got["iters"] == -1)[0]
    assert len(unwritten) == 0, (what, "jobs no wavefront wrote", unwritten[:10])
    bad = np.nonzero((got["ok"] != ref["ok"]) | (got["iters"] != ref["iters"]) | (_bits(got["u"]) != _bits(ref["u"])).any(1))[0]
    if len(bad):
        k = int(bad[0])
        detail = dict(job=k, got=(got["u"][k].tolist(), int(got["ok"][k]), int(got["iters"][k])),
                      ref=(ref["u"][k].tolist(), int(ref["ok"][k]), int(ref["iters"][k])))
        raise AssertionError("%s: %d of %d keypoints differ, first %r" % (what, len(bad), n, detail))


def _run(ctx, modsx, dplanes, plane_of, xyspd, ref, chunk, **params):
    """variant 3 at `chunk` wavefronts per range against `ref` (the oracle's answers for the list) and against variant 0"""
    _latch()
    n = len(plane_of)
    par = modsx.default_hessaff_params(**params)
    got = ctx.debug_baumberg(dplanes, plane_of, xyspd, par, variant=3, chunk=chunk)
    g = got["geometry"]
    what = "variant 3, n %d, %d wavefronts per range (asked %d) %r" % (n, g["chunk"], chunk, params)
    assert g == ctx.baumberg_geometry(n, 19, 3, chunk), what
    assert g["kernel"] == 3 and g["nchunks"] == 8 and g["grid"] == 8 * g["chunk"], what
    if chunk:
        assert g["chunk"] == chunk and g == modsx.baumberg_geometry(n, 19, 3, chunk), what
    else:
        # one resident set of wavefronts, never more than ceil(n / 2), rounded up to a multiple of 8
        resident = ctx.baumberg_geometry(1 << 30, 19, 3, 0)["grid"]
        assert resident >= 8 and g["grid"] == 8 * ((min(resident, (n + 1) // 2) + 7) // 8), (what, resident)
    if n:
        _same(got, ref, what + " against the oracle")
        _same(got, ctx.debug_baumberg(dplanes, plane_of, xyspd, par, variant=0), what + " against variant 0")
    assert got["handed_out"] == n, (what, got["handed_out"])
    return got


def test_host_geometry(ctx, modsx):
    """the host-only function answers for a forced chunk and cannot answer for the production rule (it knows no device)"""
    assert modsx.baumberg_geometry(1295, 19, 3, 5) == dict(kernel=3, chunk=5, nchunks=8, grid=40)
    assert modsx.baumberg_geometry(0, 19, 3, 5) == dict(kernel=3, chunk=5, nchunks=8, grid=40)
    for bad in (dict(W=11, chunk=5), dict(chunk=0), dict(chunk=-1), dict(chunk=(1 << 20) + 1)):
        with pytest.raises(RuntimeError):
            modsx.baumberg_geometry(1295, **dict(dict(W=19, variant=3), **bad))
    with pytest.raises(RuntimeError):
        ctx.baumberg_geometry(1295, 11, 3, 0)
    resident = ctx.baumberg_geometry(1 << 30, 19, 3, 0)["grid"]
    print("resident wavefronts of the queue form on this device:", resident)
    assert resident % 8 == 0 and ctx.baumberg_geometry(57584, 19, 3, 0)["grid"] == min(resident, 57584 // 2)
    assert ctx.baumberg_geometry(0, 19, 3, 0) == dict(kernel=3, chunk=0, nchunks=8, grid=0)
    for variant in (0, 1, 2):            # the other variants: the context's answer is the module's
        assert ctx.baumberg_geometry(1295, 19, variant, 0) == modsx.baumberg_geometry(1295, 19, variant, 0)


@pytest.mark.parametrize("chunk", [0, 1, 3, 8, 400])
def test_whole_list(ctx, modsx, oracle, dplanes, chunk):
    po, xy = BC.jobs()
    _run(ctx, modsx, dplanes, po, xy, BC.oracle_results(oracle), chunk)


@pytest.mark.parametrize("chunk", [0, 1, 3])
def test_prefixes(ctx, modsx, oracle, dplanes, chunk):
    for n in (0, 1, 2, 7, 8, 9, 17):
        po, xy = BC.subset(n)
        ref = BC.oracle_results(oracle, po, xy) if n else None
        got = _run(ctx, modsx, dplanes, po, xy, ref, chunk)
        assert len(got["ok"]) == n


@pytest.mark.parametrize("chunk", [0, 1, 8])
def test_front_loaded_list(ctx, modsx, oracle, dplanes, chunk):
    base = BC.oracle_results(oracle)
    order = QM.front_loaded_order(base["reason"])
    po, xy = BC.jobs()
    ref = {f: base[f][order] for f in ("u", "ok", "iters")}           # a keypoint's answer does not depend on its place in the list
    assert (ref["iters"][:len(order) // 8] == 16).all() and (ref["ok"][:len(order) // 8] == 0).all()
    _run(ctx, modsx, dplanes, po[order], xy[order], ref, chunk)


@pytest.mark.parametrize("chunk", [0, 1])
@pytest.mark.parametrize("iters", [0, 1])
def test_iteration_caps(ctx, modsx, oracle, dplanes, iters, chunk):
    po, xy = BC.jobs()
    got = _run(ctx, modsx, dplanes, po, xy, BC.oracle_results(oracle, po, xy, maxIterations=iters), chunk, maxIterations=iters)
    if iters == 0:
        assert (got["iters"] == 0).all() and (got["ok"] == 0).all() and (got["u"] == np.array([1, 0, 0, 1], np.float32)).all()


@pytest.fixture(scope="module")
def in_process(ctx, modsx, small_pair):
    _latch()
    return modsx.baumberg_production_variant(19), QC.detect(modsx, ctx, small_pair[:2])


@pytest.mark.parametrize("queue", ["0", "1"])
def test_production_switch(modsx, in_process, queue, tmp_path):
    """detect_affine_keypoints with the queue form forced off / on in a child process against this process (whichever it runs)"""
    global _FAULT
    _latch()
    here_variant, here = in_process
    assert here_variant == {"0": 0, "1": 3}.get(os.environ.get("MODSX_BAUMBERG_QUEUE"), here_variant) and here_variant in (0, 3)
    outp = str(tmp_path / "out.npz")
    env = dict(os.environ, MODSX_BAUMBERG_QUEUE=queue)
    try:
        p = subprocess.run([sys.executable, CHILD, outp], env=env, timeout=CHILD_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except subprocess.TimeoutExpired as e:
        _FAULT = ("did not end within %d s" % CHILD_TIMEOUT_S, (e.stderr or b"").decode(errors="replace")[-1500:])
        _latch()
    err = p.stderr.decode(errors="replace")
    if p.returncode < 0 or p.returncode in (134, 139) or (p.returncode != 0 and any(m in err.lower() for m in HIP_ERROR_MARKS)):
        _FAULT = ("ended with status %d" % p.returncode, err[-1500:])
        _latch()
    assert p.returncode == 0, "the child failed with status %d:\n%s" % (p.returncode, err[-1500:])
    z = np.load(outp)
    assert int(z["variant"]) == (3 if queue == "1" else 0)
    assert len(here) == 4 and min(len(r) for r in here) > 20
    for i, r in enumerate(here):
        assert same_records(z["k%d" % i].view(modsx.KEYPOINT), r), (queue, i)
