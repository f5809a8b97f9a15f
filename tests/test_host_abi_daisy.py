"""CPU: the entries of the DAISY descriptor exist in the library with the argument lists of include/modsx.h, and what needs no
device -- the width, the tables and the refusals that come before any context is touched -- behaves as the header says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

REGIONS = ["modsx_ctx*", "constmodsx_image*", "constmodsx_region*", "int", "double", "int", "int", "int"]
DAISY = ["int", "int", "int", "int", "int"]            # rad, radq, thq, histq, nrm_type
# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_daisy_dim": ["int", "int", "int"],
    "modsx_daisy_patches": ["modsx_ctx*", "constfloat*", "int", "int"] + DAISY + ["float*"],
    "modsx_daisy_patches_device": ["modsx_ctx*", "constvoid*", "int", "int"] + DAISY + ["void*"],
    "modsx_describe_regions_daisy": REGIONS + DAISY + ["float*"],
    "modsx_describe_regions_daisy_device": REGIONS + DAISY + ["void*"],
    "modsx_daisy_tables": ["int", "int", "int", "int", "float*", "float*", "float*", "int*", "float*", "int*", "int*", "int*", "float*"],
    "modsx_daisy_counters": ["modsx_ctx*", "long*", "int"],
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
    assert re.search(r"#define\s+MODSX_DAISY_MAX_DIM\s+200\b", hdr) and modsx.DAISY_MAX_DIM == 200
    assert re.search(r"#define\s+MODSX_DAISY_MAX_TAPS\s+51\b", hdr) and modsx.DAISY_MAX_TAPS == 51
    for method in ("daisy_patches", "daisy_patches_device", "describe_regions_daisy", "describe_regions_daisy_device", "daisy_counters"):
        assert callable(getattr(modsx.Context, method))
    assert callable(modsx.daisy_tables) and callable(modsx.daisy_dim) and modsx.DAISY_COUNTERS == ("calls", "patches", "sub_batches")


def test_argument_names_mirror_the_surf_block():
    """the region entries put rad, radq, thq, histq, nrm_type between SURF's arguments and the output, the patch entries behind
    patchSize"""
    hdr = _header()
    names = lambda fn: [re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", p).group(1) for p in _params(fn, hdr)]      # noqa: E731
    daisy = ["rad", "radq", "thq", "histq", "nrm_type"]
    surf = names("modsx_describe_regions_surf")
    assert names("modsx_describe_regions_daisy") == surf[:-1] + daisy + surf[-1:]
    surf = names("modsx_describe_regions_surf_device")
    assert names("modsx_describe_regions_daisy_device") == surf[:-1] + daisy + surf[-1:]
    assert names("modsx_daisy_patches") == ["ctx", "patches", "n", "patchSize"] + daisy + ["desc"]
    assert names("modsx_daisy_patches_device") == ["ctx", "dev_patches", "n", "patchSize"] + daisy + ["dev_desc"]
    assert names("modsx_daisy_dim") == ["radq", "thq", "histq"]


def test_daisy_dim(modsx):
    L = modsx.lib()
    assert modsx.daisy_dim() == 200 == L.modsx_daisy_dim(3, 8, 8)
    for radq in (1, 2, 3):
        for thq in range(1, 9):
            assert L.modsx_daisy_dim(radq, thq, 8) == (radq * thq + 1) * 8 <= modsx.DAISY_MAX_DIM
    for radq, thq, histq in ((0, 8, 8), (4, 8, 8), (3, 0, 8), (3, 9, 8), (3, 8, 7), (3, 8, 9), (3, 8, 0), (-1, 8, 8), (3, -8, 8)):
        assert L.modsx_daisy_dim(radq, thq, histq) == -1, (radq, thq, histq)
        assert L.modsx_last_error()
    with pytest.raises(RuntimeError, match="radq"):
        modsx.daisy_dim(radq=4)


def test_tables(modsx):
    L = modsx.lib()
    t = modsx.daisy_tables()
    assert list(t["fsz"]) == [7, 13, 21, 27] and list(t["selected"]) == [0, 1, 2]
    assert t["taps"].shape == (4, 51) and t["w"].shape == (25, 4) and (t["state"] == modsx.DAISY_SAMPLED).all()
    for f, n in enumerate(t["fsz"]):
        taps = t["taps"][f, :n]
        assert abs(float(taps.sum()) - 1) < 1e-6 and taps.argmax() == n // 2 and not t["taps"][f, n:].any()
    assert abs(float(t["k5"].sum()) - 1) < 1e-6 and t["k5"].argmax() == 2
    # the layer directions: l * 45 degrees
    ang = np.arange(8) * np.pi / 4
    assert np.abs(t["kos"] - np.cos(ang)).max() < 1e-6 and np.abs(t["zin"] - np.sin(ang)).max() < 1e-6
    assert t["kos"][0] == 1 and t["zin"][0] == 0
    # the centre reads pixel (20, 20) alone; ring r, point t sits at radius (r + 1) * 5 and angle t * 45 degrees
    assert t["base"][0] == 20 * 41 + 20 and list(t["w"][0]) == [1, 0, 0, 0]
    assert np.abs(t["w"].sum(1) - 1).max() < 1e-6 and t["w"].min() > -1e-6         # w3 = 1 + w0 - alpha - beta may round below 0
    for r in range(3):
        for k in range(8):
            g = 1 + 8 * r + k
            y, x = divmod(int(t["base"][g]), 41)
            cx, cy = 20 + 5 * (r + 1) * np.cos(ang[k]), 20 + 5 * (r + 1) * np.sin(ang[k])
            assert abs(x + (t["w"][g][1] + t["w"][g][3]) - cx) < 1e-4 and abs(y + (t["w"][g][2] + t["w"][g][3]) - cy) < 1e-4, g
    # rad = 20: the points of the outer ring at +x and +y give zeros; one ring of radius 20: they are outside [0, 40)
    assert list(np.nonzero(modsx.daisy_tables(20, 3, 8, 8)["state"] != modsx.DAISY_SAMPLED)[0]) == [17, 19]
    assert list(modsx.daisy_tables(20, 1, 8, 8)["state"][[1, 3]]) == [modsx.DAISY_SKIPPED] * 2
    assert list(modsx.daisy_tables(20, 1, 8, 8)["fsz"]) == [7, 51] and list(modsx.daisy_tables(1, 3, 8, 8)["fsz"]) == [7, 3, 3, 3]
    # any pointer may be left out
    fsz = np.zeros(4, np.int32)
    none = [None] * 9
    assert L.modsx_daisy_tables(15, 3, 8, 8, None, None, None, fsz.ctypes.data_as(C.c_void_p), *none[4:]) == 0 and list(fsz) == [7, 13, 21, 27]
    assert L.modsx_daisy_tables(15, 3, 8, 8, *none) == 0


def test_refusals_without_a_device(modsx):
    L = modsx.lib()
    none = [None] * 9
    bad = {"histq": ((15, 3, 8, 7), (15, 3, 8, 9), (15, 3, 8, 0), (15, 3, 8, 16)), "thq": ((15, 3, 0, 8), (15, 3, 9, 8), (15, 3, -1, 8)),
           "radq": ((15, 0, 8, 8), (15, 4, 8, 8), (15, -3, 8, 8)), "rad": ((0, 3, 8, 8), (21, 3, 8, 8), (-15, 3, 8, 8), (1 << 20, 3, 8, 8))}
    for word, sets in bad.items():
        for P in sets:
            assert L.modsx_daisy_tables(*P, *none) == -1, P
            assert word.encode() in L.modsx_last_error(), (P, L.modsx_last_error())
    for P in ((1, 1, 1, 8), (20, 3, 8, 8)):                                    # the bounds themselves
        assert L.modsx_daisy_tables(*P, *none) == 0, P
    buf = np.zeros(1681, np.float32).ctypes.data_as(C.c_void_p)
    # a null context is refused before anything else is looked at
    assert L.modsx_daisy_patches(None, buf, 1, 41, 15, 3, 8, 8, 0, buf) == -1
    assert L.modsx_daisy_patches_device(None, buf, 1, 41, 15, 3, 8, 8, 0, buf) == -1
    assert L.modsx_describe_regions_daisy(None, buf, buf, 1, C.c_double(5.1962), 41, 0, 1, 15, 3, 8, 8, 0, buf) == -1
    assert L.modsx_describe_regions_daisy_device(None, buf, buf, 1, C.c_double(5.1962), 41, 0, 1, 15, 3, 8, 8, 0, buf) == -1
    assert L.modsx_daisy_counters(None, buf, 3) == -1
    assert b"null argument" in L.modsx_last_error()


def test_refusals_of_the_entries_come_before_the_context_is_used(modsx):
    """nrm_type 3 and patchSize 40 (and every range above) are refused by the patch and region entries on a context handle that is
    never dereferenced: the argument checks come first, so this needs no device"""
    L = modsx.lib()
    fake = C.create_string_buffer(1 << 16)             # zero bytes standing in for a context; a refusal must not touch it
    h = C.cast(fake, C.c_void_p)
    buf = np.zeros(1681, np.float32).ctypes.data_as(C.c_void_p)
    mr = C.c_double(5.1962)
    bad = (("nrm_type", (41, 15, 3, 8, 8, 3)), ("nrm_type", (41, 15, 3, 8, 8, -1)), ("patchSize", (40, 15, 3, 8, 8, 0)),
           ("patchSize", (42, 15, 3, 8, 8, 0)), ("histq", (41, 15, 3, 8, 4, 0)), ("thq", (41, 15, 3, 0, 8, 0)), ("thq", (41, 15, 3, 9, 8, 0)),
           ("radq", (41, 15, 0, 8, 8, 0)), ("radq", (41, 15, 4, 8, 8, 0)), ("rad", (41, 0, 3, 8, 8, 0)), ("rad", (41, 21, 3, 8, 8, 0)))
    for word, (ps, rad, radq, thq, histq, nrm) in bad:
        for rc in (L.modsx_daisy_patches(h, buf, 1, ps, rad, radq, thq, histq, nrm, buf),
                   L.modsx_daisy_patches_device(h, buf, 1, ps, rad, radq, thq, histq, nrm, buf),
                   L.modsx_describe_regions_daisy(h, buf, buf, 1, mr, ps, 0, 1, rad, radq, thq, histq, nrm, buf),
                   L.modsx_describe_regions_daisy_device(h, buf, buf, 1, mr, ps, 0, 1, rad, radq, thq, histq, nrm, buf)):
            assert rc == -1 and word.encode() in L.modsx_last_error(), (word, rc, L.modsx_last_error())
    assert not any(fake.raw)
