"""CPU: the orientation hooks exist in the library with the argument lists of include/modsx.h, and what needs no device -- the
tables and the launch counters' reset -- behaves as the header says."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

# name -> the C parameter types of include/modsx.h, whitespace removed
DECLARED = {
    "modsx_debug_orientation_counts": ["unsignedlonglong*", "unsignedlonglong*", "int"],
    "modsx_debug_orientation_launches": ["unsignedlonglong*", "unsignedlonglong*", "int"],
    "modsx_orientation_tables": ["unsignedchar*", "unsignedshort*", "float*", "unsignedshort*", "float*", "int*"],
}


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
        bound = ["ptr" if t is C.c_void_p else "int" for t in getattr(L, name).argtypes]
        assert bound == ["ptr" if w.endswith("*") else w for w in want], (name, bound)
    assert callable(modsx.orientation_launches) and callable(modsx.orientation_tables) and callable(modsx.orientation_counts)


def test_tables_any_pointer_may_be_left_out(modsx):
    L = modsx.lib()
    assert L.modsx_orientation_tables(None, None, None, None, None, None) == 0
    k = np.zeros(4, np.int32)
    assert L.modsx_orientation_tables(None, None, None, None, None, k.ctypes.data_as(C.c_void_p)) == 0
    assert list(k) == [1245, 1344, 44, 8192]
    tab = np.full(2049 + 8, 0xAB, np.uint8)
    assert L.modsx_orientation_tables(tab.ctypes.data_as(C.c_void_p), None, None, None, None, None) == 0
    assert (tab[2049:] == 0xAB).all() and tab[2048] == 18                 # 2049 entries are written, no more
    t = modsx.orientation_tables()
    assert np.array_equal(t["bin_table"], tab[:2049])
    assert sorted(t) == sorted(["bin_table", "index_raster", "weight_raster", "index_lanes", "weight_lanes", "n_real", "length",
                                "stride", "global_table_from"])


def test_launch_counters_read_and_reset_without_a_device(modsx):
    a = modsx.orientation_launches(reset=True)
    assert len(a) == 2
    assert modsx.orientation_launches() == (0, 0)
    L = modsx.lib()
    x = C.c_ulonglong(7)
    assert L.modsx_debug_orientation_launches(None, C.byref(x), 0) == 0 and x.value == 0
    assert L.modsx_debug_orientation_launches(C.byref(x), None, 1) == 0 and x.value == 0
    assert L.modsx_debug_orientation_launches(None, None, 1) == 0
