"""CPU: the ABI of the stored image representations (include/modsx.h: modsx_rep_*, modsx_match_reps, modsx_match_one_to_many)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["modsx_rep_create", "modsx_rep_free", "modsx_rep_add_views", "modsx_rep_append", "modsx_rep_class", "modsx_rep_match_fginn",
       "modsx_match_reps", "modsx_match_one_to_many"]


def test_representation_symbols_are_declared_listed_and_exported(modsx):
    hdr = open(os.path.join(ROOT, "include", "modsx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(modsx_[a-z0-9_]+)\s*\(", hdr))
    L = modsx.lib()
    for name in NEW:
        assert name in declared, name
        assert name in modsx.EXPORTS, name
        assert hasattr(L, name), name
    assert re.search(r"typedef\s+struct\s*\{\s*int\s+detector\s*,\s*desc_type\s*;\s*double\s+ratio\s*;\s*\}\s*modsx_rep_class_sel\s*;", hdr)
    assert C.sizeof(modsx.RepClassSel) == 16
    for name in ("Rep", "match_reps", "match_one_to_many"):
        assert hasattr(modsx, name), name
    for name in ("add_views", "append", "regions", "free"):
        assert hasattr(modsx.Rep, name), name
    assert hasattr(modsx.Context, "rep_match_fginn")


def test_existing_structs_keep_their_size_and_the_version_stays(modsx):
    # modsx_pair_params / modsx_pair_result as they were before the representations came (x86-64 SysV)
    assert C.sizeof(modsx.PairParams) == 328
    assert C.sizeof(modsx.PairResult) == 128
    assert C.sizeof(modsx.LadderStep) == 80
    assert modsx.lib().modsx_version() == 100
