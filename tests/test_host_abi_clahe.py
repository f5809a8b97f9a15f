"""CPU: the C boundary of CLAHE (include/modsx.h: the drivers' doCLAHE step) -- the argument lists of the new symbols as the
header declares them, the defaults, and every refusal that needs no device.  Parameters are checked before the context and the
images are looked at, so the entries are called here without either."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1

SYMBOLS = {
    "modsx_default_clahe_params": ("void", "modsx_clahe_params *p"),
    "modsx_image_clahe": ("int", "modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par, modsx_image *out"),
    "modsx_image_clahe_new": ("modsx_image *", "modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par"),
    "modsx_image_clahe_batch": ("int", "modsx_ctx *ctx, const modsx_image *const *in, modsx_image *const *out, int n, "
                                       "const modsx_clahe_params *par"),
    "modsx_clahe_geometry": ("int", "int rows, int cols, const modsx_clahe_params *par, int *out"),
    "modsx_debug_clahe": ("int", "modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par, int *hist, unsigned char *lut"),
    "modsx_clahe_counters": ("int", "modsx_ctx *ctx, long *out, int n"),
}


def _err(modsx):
    return modsx.lib().modsx_last_error().decode()


def test_declared_argument_lists(modsx):
    hdr = open(os.path.join(ROOT, "include", "modsx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, (ret, args) in SYMBOLS.items():
        m = re.search(r"(\b(?:int|void)\s+|\bmodsx_image\s*\*\s*)%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        assert "".join(m.group(1).split()) == "".join(ret.split()), name
        assert " ".join(m.group(2).split()) == " ".join(args.split()), name
        assert name in modsx.EXPORTS and hasattr(modsx.lib(), name)
    m = re.search(r"typedef struct modsx_clahe_params \{(.*?)\} modsx_clahe_params;", hdr, re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"\b(int|double)\s+([\w\s,]+);", m.group(1)) for n in names.split(",")]
    assert fields == [("double", "clip_limit"), ("int", "tiles_x"), ("int", "tiles_y"), ("int", "variant")]
    assert [(n, {C.c_double: "double", C.c_int: "int"}[t]) for n, t in modsx.ClaheParams._fields_] == [(n, t) for t, n in fields]
    assert C.sizeof(modsx.ClaheParams) == 24
    assert re.search(r"#define\s+MODSX_CLAHE_MAX_TILES\s+256\b", hdr) and modsx.CLAHE_MAX_TILES == 256
    assert len(modsx.CLAHE_COUNTERS) == 6 and len(modsx.CLAHE_GEOMETRY) == 9


def test_defaults_are_what_the_drivers_set(modsx):
    p = modsx.ClaheParams()
    modsx.lib().modsx_default_clahe_params(C.byref(p))
    assert (p.clip_limit, p.tiles_x, p.tiles_y, p.variant) == (4.0, 8, 8, 0)      # createCLAHE(); setClipLimit(4)
    modsx.lib().modsx_default_clahe_params(None)                                  # tolerated
    q = modsx.clahe_params(clip_limit=40.0, tiles=(3, 5), variant=1)
    assert (q.clip_limit, q.tiles_x, q.tiles_y, q.variant) == (40.0, 3, 5, 1)


BAD = [(dict(tiles=(0, 8)), "tiles"), (dict(tiles=(8, -2)), "tiles"), (dict(tiles=(32, 9)), "256"), (dict(tiles=(65536, 65536)), "256"),
       (dict(clip_limit=-0.5), "clip_limit"), (dict(clip_limit=float("nan")), "clip_limit"), (dict(clip_limit=float("inf")), "clip_limit"),
       (dict(variant=2), "variant"), (dict(variant=-1), "variant")]


@pytest.mark.parametrize("kw,word", BAD)
def test_parameter_refusals_need_no_device(modsx, kw, word):
    L, p = modsx.lib(), modsx.clahe_params(**kw)
    one = (C.c_void_p * 1)(None)
    hist, lut = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    for call in (lambda: L.modsx_image_clahe(None, None, C.byref(p), None),
                 lambda: L.modsx_image_clahe_batch(None, one, one, 1, C.byref(p)),
                 lambda: L.modsx_image_clahe_batch(None, None, None, 0, C.byref(p)),        # also when nothing would be launched
                 lambda: L.modsx_debug_clahe(None, None, C.byref(p), hist.ctypes.data_as(C.c_void_p), lut.ctypes.data_as(C.c_void_p)),
                 lambda: L.modsx_clahe_geometry(64, 64, C.byref(p), np.zeros(9, np.int32).ctypes.data_as(C.c_void_p))):
        assert call() == ERR_ARG and word in _err(modsx), _err(modsx)
    assert L.modsx_image_clahe_new(None, None, C.byref(p)) is None and word in _err(modsx)


def test_null_pointers(modsx):
    L, p = modsx.lib(), modsx.clahe_params()
    out = np.zeros(9, np.int32)
    assert L.modsx_clahe_geometry(64, 64, None, out.ctypes.data_as(C.c_void_p)) == ERR_ARG and "par" in _err(modsx)
    assert L.modsx_clahe_geometry(64, 64, C.byref(p), None) == ERR_ARG
    assert L.modsx_image_clahe(None, None, None, None) == ERR_ARG and "par" in _err(modsx)
    assert L.modsx_image_clahe(None, None, C.byref(p), None) == ERR_ARG and "ctx" in _err(modsx)
    assert L.modsx_image_clahe_new(None, None, None) is None and "par" in _err(modsx)
    assert L.modsx_image_clahe_new(None, None, C.byref(p)) is None
    assert L.modsx_image_clahe_batch(None, None, None, 1, C.byref(p)) == ERR_ARG and "ctx" in _err(modsx)
    assert L.modsx_image_clahe_batch(None, None, None, -1, C.byref(p)) == ERR_ARG
    assert L.modsx_image_clahe_batch(None, None, None, 0, None) == ERR_ARG
    assert L.modsx_image_clahe_batch(None, None, None, 0, C.byref(p)) == 0        # an empty batch is no work and no error
    assert L.modsx_debug_clahe(None, None, C.byref(p), None, None) == ERR_ARG and "ctx" in _err(modsx)
    assert L.modsx_clahe_counters(None, None, 0) == ERR_ARG


def test_geometry_through_the_c_entry(modsx):
    out = np.zeros(9, np.int32)
    p = modsx.clahe_params()
    assert modsx.lib().modsx_clahe_geometry(768, 1024, C.byref(p), out.ctypes.data_as(C.c_void_p)) == 9
    assert out[:5].tolist() == [128, 96, 1024, 768, 192]
    assert out[5:6].view(np.float32)[0] == np.float32(255.0) / np.float32(12288)
    assert out[6:].tolist() == [3, 32, 192]
