"""CPU: the entries of the KAZE detector exist in the library with the argument lists of include/modsx.h, and what needs no device
-- the level and tau tables (against the fixture of the compiled reference), kaze_regions and the refusals that come before any
context is touched -- behaves as the header says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kaze_cases as KC
import kaze_model as M
from conftest import ROOT

PAR = "constmodsx_kaze_params*"
PT = "modsx_kaze_point*"
# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_detect_kaze": ["modsx_ctx*", "constmodsx_image*", PAR, "modsx_keypoint**"],
    "modsx_detect_kaze_batch": ["modsx_ctx*", "constmodsx_image*const*", "int", PAR, "modsx_keypoint**", "int*"],
    "modsx_kaze_regions": ["constmodsx_keypoint*", "int", "int", "modsx_region*"],
    "modsx_kaze_geometry": ["int", "int", PAR, "int*", "float*", "float*", "int*", "int*"],
    "modsx_debug_kaze": ["modsx_ctx*", "constmodsx_image*", PAR, "float*", "long*", "float*", "float*", "float*", "float*", "int*", "float*",
                         PT, PT, PT, "int", "int*"],
    "modsx_debug_kaze_scan": ["modsx_ctx*", "int", "int", PAR, "constfloat*", "int*", "float*", PT, PT, PT, "int", "int*"],
    "modsx_kaze_counters": ["modsx_ctx*", "long*", "int"],
}
FIELDS = ["omax", "nsublevels", "soffset", "derivative_factor", "dthreshold", "min_dthreshold", "kcontrast_percentile", "kcontrast_nbins",
          "descriptor", "diffusivity"]


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "kaze_ref.npz"))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modsx.h")).read(), flags=re.S)


def _params(name, hdr):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_symbols_exist_with_the_headers_argument_lists(modsx):
    hdr = _header()
    L = modsx.lib()
    for name, want in DECLARED.items():
        params = [re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", p).replace(" ", "") for p in _params(name, hdr)]
        assert params == want, (name, params)
        assert name in modsx.EXPORTS and hasattr(L, name), name
        bound = [{C.c_void_p: "ptr", C.c_int: "int"}[t] for t in getattr(L, name).argtypes]
        assert bound == ["ptr" if w.endswith("*") else w for w in want], (name, bound)
    assert "modsx_default_kaze_params" in modsx.EXPORTS and hasattr(L, "modsx_default_kaze_params")
    assert re.search(r"#define\s+MODSX_DET_KAZE\s+9\b", hdr) and modsx.DET_KAZE == 9 == M.DET_KAZE
    assert re.search(r"#define\s+MODSX_KAZE_MAX_LEVELS\s+32\b", hdr) and modsx.KAZE_MAX_LEVELS == 32
    assert re.search(r"#define\s+MODSX_KAZE_MAX_TAU\s+64\b", hdr) and modsx.KAZE_MAX_TAU == 64
    m = re.search(r"typedef struct modsx_kaze_params \{(.*?)\} modsx_kaze_params;", hdr, flags=re.S)
    names = re.findall(r"([a-z_]+)\s*[,;]", m.group(1))
    assert names == FIELDS == [f[0] for f in modsx.KazeParams._fields_]
    assert C.sizeof(modsx.KazeParams) == 40 and modsx.KAZE_POINT.itemsize == 24
    m = re.search(r"typedef struct modsx_kaze_point \{(.*?)\} modsx_kaze_point;", hdr, flags=re.S)
    assert re.findall(r"([a-z_]+)\s*[,;]", m.group(1)) == list(modsx.KAZE_POINT.names) == list(M.KP.names)
    for method in ("detect_kaze", "detect_kaze_batch", "debug_kaze", "debug_kaze_scan", "kaze_counters"):
        assert callable(getattr(modsx.Context, method))
    assert len(modsx.KAZE_COUNTERS) == 9 and modsx.KAZE_COUNTERS[-1] == "filter_us"


def test_default_parameters(modsx):
    p = modsx.kaze_params()
    got = {f: getattr(p, f) for f in FIELDS}
    want = dict(M.DEFAULTS, diffusivity=1)
    for f in FIELDS:
        assert np.float32(got[f]) == np.float32(want[f]), (f, got[f], want[f])


def test_geometry_against_the_fixtures_level_and_tau_tables(modsx, fixture):
    """the level table of Allocate_Memory_Evolution and every tau list of fed_tau_by_process_time, as the compiled reference has
    them, for every case's size and parameters; the tile sizes and the surviving octaves"""
    seen = set()
    for k, (name, img, par) in enumerate(KC.cases()):
        g = modsx.kaze_geometry(img.shape[0], img.shape[1], modsx.kaze_params(**par))
        ref, sig, tau = fixture["c%02d_levels" % k], fixture["c%02d_sigmas" % k], fixture["c%02d_tau" % k]
        lv = g["levels"]
        # fixture rows: octave, sublevel, rows, cols, sigma_size, FED steps
        assert np.array_equal(lv[:, :5], ref[:, :5]) and np.array_equal(lv[:, 7], ref[:, 5]), name
        assert g["sigmas"].tobytes() == sig.tobytes(), name
        for i, t in enumerate(g["tau"]):
            assert t.tobytes() == tau[i, :len(t)].tobytes(), (name, i)
        assert g["omax"] == int(fixture["c%02d_omax" % k]) == lv[-1, 0] + 1, name
        assert np.array_equal(lv[:, 5], 3 + 2 * (lv[:, 6] - 1))
        assert g["tiles"] == dict(width=64, height=16, scan=256, max_distance=8)
        seen.add(g["omax"])
        if name in KC.OCTAVES:
            assert g["omax"] == KC.OCTAVES[name], name
    assert seen == {1, 2, 3, 4}
    # the defaults: derivative distances 2, 3, 3, 4 in every octave and 166 steps over 16 levels
    g = modsx.kaze_geometry(320, 640)
    assert list(g["levels"][:, 6]) == [2, 3, 3, 4] * 4 and int(g["levels"][:, 7].sum()) == 166 and len(g["levels"]) == 16
    # NULL outputs are allowed
    p = modsx.kaze_params()
    assert modsx.lib().modsx_kaze_geometry(96, 128, C.byref(p), None, None, None, None, None) == 4


def test_kaze_regions(modsx):
    final = np.zeros(3, M.KP)
    final["x"], final["y"], final["size"], final["response"] = (10.5, 20.25, 30), (7, 8, 9.5), (4.8, 9.6, 19.2), (0.01, 0.02, 0.03)
    final["octave"], final["class_id"] = (0, 1, 2), (0, 4, 8)
    kps = M.keypoints(final, modsx.KEYPOINT)
    assert kps["s"][0] == float(np.float32(4.8)) / 3.0 and list(kps["octave_number"]) == [0, 1, 2]
    regs = modsx.kaze_regions(kps, img_id=5)
    assert len(regs) == 3 and np.all(regs["type"] == 9) and np.all(regs["img_id"] == 5) and list(regs["id"]) == [0, 1, 2]
    assert np.all(regs["img_reproj_id"] == 0) and np.all(regs["parent_id"] == 0)
    for f in modsx.KEYPOINT.names:
        assert regs["det_kp"][f].tobytes() == kps[f].tobytes(), f
        assert not regs["reproj_kp"][f].any()
    assert len(modsx.kaze_regions(kps[:0])) == 0
    L = modsx.lib()
    assert L.modsx_kaze_regions(None, 2, 0, None) == -1 and L.modsx_kaze_regions(None, -1, 0, None) == -1


def test_refusals_that_need_no_device(modsx):
    L = modsx.lib()
    bad = [dict(diffusivity=0), dict(diffusivity=2), dict(diffusivity=3), dict(omax=0), dict(omax=9), dict(nsublevels=0),
           dict(omax=8, nsublevels=5), dict(soffset=0.0), dict(derivative_factor=0.0), dict(derivative_factor=9.0), dict(kcontrast_nbins=0),
           dict(kcontrast_nbins=5000), dict(descriptor=6), dict(descriptor=-1)]
    for kw in bad:
        p = modsx.kaze_params(**kw)
        assert L.modsx_kaze_geometry(96, 128, C.byref(p), None, None, None, None, None) == -1, kw
        msg = L.modsx_last_error()
        assert msg.startswith(b"modsx_kaze_geometry: "), msg
        if "diffusivity" in kw:
            assert b"PM_G2" in msg and b"exp / pow" in msg, msg
        with pytest.raises(RuntimeError):
            modsx.kaze_geometry(96, 128, p)
    p = modsx.kaze_params()
    for rows, cols in ((2, 100), (100, 2), (0, 0), (-1, 5)):
        assert L.modsx_kaze_geometry(rows, cols, C.byref(p), None, None, None, None, None) == -1 and b"3 x 3" in L.modsx_last_error()
    assert L.modsx_kaze_geometry(96, 128, None, None, None, None, None, None) == -1
    out, cnt = C.c_void_p(), (C.c_int * 2)()
    assert L.modsx_detect_kaze(None, None, C.byref(p), C.byref(out)) == -1
    assert L.modsx_detect_kaze_batch(None, None, 0, C.byref(p), C.byref(out), cnt) == -1
    assert L.modsx_kaze_counters(None, None, 0) == -1
    with pytest.raises(TypeError):
        modsx.kaze_params(octaves=3)
