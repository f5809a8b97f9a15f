"""CPU: the entries of the SURF detector exist in the library with the argument lists of include/modsx.h, and what needs no device
-- the layer table, the parameter normalisation, surf_regions and the refusals that come before any context is touched -- behaves
as the header says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surfdet_model as M
from conftest import ROOT

PAR = "constmodsx_surfdet_params*"
# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_detect_surf": ["modsx_ctx*", "constmodsx_image*", PAR, "modsx_keypoint**"],
    "modsx_detect_surf_batch": ["modsx_ctx*", "constmodsx_image*const*", "int", PAR, "modsx_keypoint**", "int*"],
    "modsx_surf_regions": ["constmodsx_keypoint*", "int", "int", "modsx_region*"],
    "modsx_surfdet_geometry": ["int", "int", PAR, "int*"],
    "modsx_surfdet_normalise": [PAR, "modsx_surfdet_params*"],
    "modsx_debug_surfdet": ["modsx_ctx*", "constmodsx_image*", PAR, "float*", "int*", "float*", "unsignedchar*", "int*", "double*", "double*",
                            "double*", "int*", "int*", "int", "int*"],
    "modsx_surfdet_counters": ["modsx_ctx*", "long*", "int"],
}


def _ctype_name(t):
    return {C.c_void_p: "ptr", C.c_int: "int", C.c_double: "double"}[t]


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
        bound = [_ctype_name(t) for t in getattr(L, name).argtypes]
        assert bound == ["ptr" if w.endswith("*") else w for w in want], (name, bound)
    assert re.search(r"#define\s+MODSX_DET_SURF\s+6\b", hdr) and modsx.DET_SURF == 6 == M.DET_SURF
    assert re.search(r"#define\s+MODSX_SURFDET_MAX_LAYERS\s+12\b", hdr) and modsx.SURFDET_MAX_LAYERS == 12 == len(M.FILTERS)
    m = re.search(r"typedef struct modsx_surfdet_params \{(.*?)\} modsx_surfdet_params;", hdr, flags=re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int octaves, intervals, init_sample; float thresh;"
    assert [f[0] for f in modsx.SurfDetParams._fields_] == ["octaves", "intervals", "init_sample", "thresh"]
    assert C.sizeof(modsx.SurfDetParams) == 16
    for method in ("detect_surf", "detect_surf_batch", "debug_surfdet", "surfdet_counters"):
        assert callable(getattr(modsx.Context, method))
    assert callable(modsx.surf_regions) and callable(modsx.surfdet_geometry)
    assert modsx.SURFDET_COUNTERS == ("calls", "images", "extrema", "accepted", "regrows")


SIZES = [(30, 30), (33, 31), (48, 63), (48, 64), (48, 65), (48, 129), (300, 239), (480, 478), (240, 320), (768, 1024), (16, 16), (96, 97),
         (6, 6), (1, 1)]
PARAMS = [dict(M.INI), dict(M.INI, init_sample=1), dict(M.INI, init_sample=3), dict(M.INI, init_sample=6), dict(M.INI, octaves=1),
          dict(M.INI, octaves=0), dict(M.INI, octaves=5), dict(M.INI, octaves=2, init_sample=0), dict(M.INI, init_sample=7)]


def test_geometry_against_the_models_layer_table(modsx):
    L = modsx.lib()
    refused = 0
    for rows, cols in SIZES:
        for par in PARAMS:
            p = modsx.surfdet_params(**par)
            try:
                want = M.geometry(rows, cols, **par)
            except ValueError:
                refused += 1
                assert L.modsx_surfdet_geometry(rows, cols, C.byref(p), None) == -1 and b"width or height 0" in L.modsx_last_error()
                with pytest.raises(RuntimeError):
                    modsx.surfdet_geometry(rows, cols, p)
                continue
            got = modsx.surfdet_geometry(rows, cols, p)
            assert got.dtype == np.int32 and np.array_equal(got, np.array(want, np.int32)), (rows, cols, par)
            assert L.modsx_surfdet_geometry(rows, cols, C.byref(p), None) == len(want)          # the table may be left out
    assert refused > 5
    # width quotient 17 between layer 0 and the w / 16 layers of a 239-wide layer 0 (layers getIpoints never pairs)
    g = modsx.surfdet_geometry(300, 239, modsx.surfdet_params(octaves=0, init_sample=1))
    assert g[0, 0] // g[-1, 0] == 17 and g[-1, 2] // g[0, 2] == 16
    assert np.array_equal(modsx.surfdet_geometry(240, 320), np.array(M.geometry(240, 320, **M.INI), np.int32))     # the ini's by default


def test_parameter_normalisation(modsx):
    for o in (-1, 0, 1, 2, 3, 4, 5, 6, 100):
        for iv in (-2, 0, 1, 4, 5):
            for s in (-1, 0, 1, 2, 6, 7):
                for t in (-1.0, -1e-30, -0.0, 0.0, 0.0004, 1e-30, 3.5, float("inf"), float("nan")):
                    got = modsx.surfdet_normalise(modsx.surfdet_params(o, iv, s, t))
                    with np.errstate(invalid="ignore"):
                        want = M.normalise(o, iv, s, t)
                    assert (got.octaves, got.intervals, got.init_sample) == want[:3], (o, iv, s, t)
                    assert np.float32(got.thresh).tobytes() == np.float32(want[3]).tobytes(), (t, got.thresh, want[3])
    d = modsx.surfdet_params()
    assert (d.octaves, d.intervals, d.init_sample, np.float32(d.thresh)) == (4, 4, 2, np.float32(0.0004))


def test_surf_regions(modsx):
    pts = np.array([[10.5, 20.25, 2.0], [0.0, 3.0, 15.5], [319.0, 1.5, 1.6]], np.float32)
    kps = M.keypoints(pts, modsx.KEYPOINT)
    assert np.signbit(kps["a21"]).all() and (kps["a21"] == 0).all() and (kps["a11"] == 1).all() and (kps["a12"] == 0).all()
    regs = modsx.surf_regions(kps, img_id=7)
    assert regs.dtype == modsx.REGION and len(regs) == 3
    assert (regs["type"] == 6).all() and (regs["img_id"] == 7).all() and list(regs["id"]) == [0, 1, 2]
    assert (regs["img_reproj_id"] == 0).all() and (regs["parent_id"] == 0).all()
    assert regs["det_kp"].tobytes() == kps.tobytes(), "det_kp as given: no scaling, no rectification"
    assert regs["reproj_kp"].tobytes() == np.zeros(3, modsx.KEYPOINT).tobytes()
    # the rest as modsx_detect_affine_regions leaves it
    aff = modsx.detect_affine_regions(kps, img_id=7, det_type=6)
    for f in ("img_id", "img_reproj_id", "id", "parent_id", "type"):
        assert np.array_equal(regs[f], aff[f]), f
    assert regs["reproj_kp"].tobytes() == aff["reproj_kp"].tobytes()
    assert len(modsx.surf_regions(kps[:0])) == 0
    L = modsx.lib()
    buf = np.zeros(1, modsx.REGION)
    assert L.modsx_surf_regions(None, 1, 0, buf.ctypes.data_as(C.c_void_p)) == -1
    assert L.modsx_surf_regions(kps.ctypes.data_as(C.c_void_p), 1, 0, None) == -1
    assert L.modsx_surf_regions(kps.ctypes.data_as(C.c_void_p), -1, 0, buf.ctypes.data_as(C.c_void_p)) == -1
    assert L.modsx_surf_regions(None, 0, 0, None) == 0


def test_refusals_without_a_device(modsx):
    L = modsx.lib()
    p = modsx.surfdet_params()
    buf = np.zeros(64, np.float64).ctypes.data_as(C.c_void_p)
    out = C.c_void_p()
    # a null context is refused before anything else is looked at
    assert L.modsx_detect_surf(None, buf, C.byref(p), C.byref(out)) == -1
    assert L.modsx_detect_surf_batch(None, buf, 1, C.byref(p), C.byref(out), buf) == -1
    assert L.modsx_debug_surfdet(None, buf, C.byref(p), buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, 1, buf) == -1
    assert L.modsx_surfdet_counters(None, buf, 5) == -1
    assert b"null argument" in L.modsx_last_error()
    assert L.modsx_surfdet_geometry(240, 320, None, None) == -1 and L.modsx_surfdet_normalise(None, C.byref(p)) == -1
    assert L.modsx_surfdet_normalise(C.byref(p), None) == -1
    for rows, cols in ((0, 10), (10, 0), (-5, 10)):
        assert L.modsx_surfdet_geometry(rows, cols, C.byref(p), None) == -1
    # 15 rows at init_sample 2: octave 4 (rows / 2 / 8) is empty; three octaves fit
    assert L.modsx_surfdet_geometry(15, 200, C.byref(p), None) == -1 and b"octave 4" in L.modsx_last_error()
    assert L.modsx_surfdet_geometry(15, 200, C.byref(modsx.surfdet_params(octaves=3)), None) == 8
