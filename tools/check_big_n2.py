#!/usr/bin/env python3
"""70 000 trains (274 pack workgroups: more than the 256 slots of a waiting workgroup's miss list) against the oracle, both branches of the walk;
with a -DMODSX_PACK_POLLS=0 build (MODSX_LIB=...) every pack workgroup counts all its predecessors itself -- the path a real run takes only when
hundreds of predecessors stay silent at once."""
import sys
sys.path.insert(0, '.')
import mods_amd
from oracle import pyoracle as O
from tests.match_cases import big_n2_case, same_tentatives      # the case tests/test_gpu_match_shapes.py runs
d1, d2, pos2, params = big_n2_case()[:4]
ctx = mods_amd.Context(0)
for ratio, cd, nn in params:
    ref = O.match_fginn(d1, d2, pos2, ratio, cd, nn); got = ctx.match_fginn(d1, d2, pos2, ratio, cd, nn)
    print("n2 = %d, ratio" % len(d2), ratio, "IDENTICAL" if same_tentatives(got, ref) else "MISMATCH", len(ref))
