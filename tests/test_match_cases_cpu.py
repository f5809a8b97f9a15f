"""CPU: the cases of tests/match_cases.py reach the paths they are meant for, and are not vacuous.

Three things are shown here, without a GPU, so that a green tests/test_gpu_match_shapes.py means what it is meant to mean:
  coverage      with the launcher's geometry restated in match_cases.layout, every one of the four shapes of k_match_sweep1 meets,
                somewhere in the tables, each split length modulo the fat shape's 16-tile stage, more than 16 streams, a ragged last
                query block, a short last split, an empty parity class, a tie run across the class boundary, splits that straddle
                the index-chunk boundaries with the planted trains on both sides.  A failure names the condition that is missing.
  model         the executable model of the decision logic (tests/match_model.py) agrees with the oracle on every small case and on
                the planted queries of the chunk cases.  Only the NUMBER of splits is taken from the case: the model cuts the packed
                tile count into S parts itself, the launcher cuts ntiles_ub, so the model's split boundaries are not the device's
                (nor match_cases.splits) -- it models the decision logic, which must hold wherever the boundaries fall.
  non-vacuity   the inputs give tentatives, and send queries through every exit of k_match_decide (conditions on the inputs: the
                oracle and the model alone decide them).
"""
import functools

import numpy as np
import pytest

from tests import match_cases as MC
from tests import match_model as M

SHAPE_IDS = ["qs%d_%s" % (qs, "fat" if fat else "thin") for qs, fat in MC.SHAPES]


def _lay(case, shape):
    return MC.layout(len(case.d1), len(case.d2), *shape)


@functools.lru_cache(None)
def _ntv(name):
    return MC.ntiles_v(_by_name(name))


@functools.lru_cache(None)
def _by_name(name):
    return {c.name: c for c in MC.small_cases() + MC.chunk_cases() + MC.big_cases()}[name]


_ORACLE = {}


def _oracle_rows(oracle, case, pi):
    """oracle tentatives of the model's queries of a case (q counts inside that subset)"""
    key = (case.name, pi)
    if key not in _ORACLE:
        sub = MC.model_queries(case)
        _ORACLE[key] = oracle.match_fginn(case.d1[sub], case.d2, case.pos2, *case.params[pi])
    return _ORACLE[key]


_MODEL = {}


def _model_rows(case, pi, S):
    key = (case.name, pi, S)
    if key not in _MODEL:
        ratio, cd, nn = case.params[pi]
        stats = []
        rows = M.match_rows(case.d1[MC.model_queries(case)], case.d2, case.pos2, ratio, cd, nn, S=S, stats=stats)
        _MODEL[key] = (M.rows_to_tentatives(rows, nn), stats)
    return _MODEL[key]


def _cmp(got, ref, what):
    """as tests/test_match_model_cpu._cmp"""
    assert len(got) == len(ref), what
    for g, r in zip(got, ref):
        assert g[:4] == (r["q"], r["t0"], r["tj"], r["t1"]), what
        assert g[4] == r["d1"] and g[5] == r["d2"] and g[6] == r["d2by2ndcl"], what
        assert g[7] == r["ratio"] or (np.isnan(g[7]) and np.isnan(r["ratio"])), what


# ---------------- coverage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MC.SHAPES, ids=SHAPE_IDS)
def test_small_table_covers_the_shape(shape):
    qs, fat = shape
    cases = MC.small_cases()
    lays = {c.name: _lay(c, shape) for c in cases}
    missing = []
    for r in (0, 4, 12):
        if not any(l["tiles_per_split"] % MC.STAGE_FAT == r for l in lays.values()):
            missing.append("a case with tilesPerSplit %% 16 == %d" % r)
    if not any(2 * l["S"] > 16 for l in lays.values()):
        missing.append("a case with more than 16 streams per query (2 S > 16)")
    if not any(l["nqb"] >= 2 and 0 < len(c.d1) - (l["nqb"] - 1) * l["qpb"] < 32 * qs for c, l in zip(cases, lays.values())):
        missing.append("two query blocks with a last block of fewer than 32 * QS queries")
    short = False
    for c in cases:
        sp = MC.splits(_ntv(c.name), lays[c.name])
        short |= len(sp) >= 2 and 0 < sp[-1][1] - sp[-1][0] < sp[0][1] - sp[0][0]
    if not short:
        missing.append("a last split that is shorter than the others and not empty")
    if not any(M.pack(c.d2)[1].min() == 1 for c in cases):
        missing.append("an empty even class")
    if not any(M.pack(c.d2)[1].max() == 0 for c in cases):
        missing.append("an empty odd class")
    # the run across the class boundary: exact ties in the last even tile, exact ties in the first odd tile, one split
    c = MC.class_boundary_case()
    tile, _ = MC.tile_of_train(c)
    tep = int((M.pack(c.d2)[1] == 0).sum())
    for q, ev, od in c.planted["runs"]:
        if not (set(tile[ev]) == {tep - 1} and set(tile[od]) == {tep} and MC.split_of(tep - 1, lays[c.name]) == MC.split_of(tep, lays[c.name])):
            missing.append("query %d: tie runs in the last even tile and the first odd tile, inside one split" % q)
        if not (np.array_equal(c.d2[ev[0]], c.d2[ev[-1]]) and np.array_equal(c.d2[od[0]], c.d2[od[-1]])
                and np.abs(c.d2[ev[0]] - c.d2[od[0]]).sum() == 1):
            missing.append("query %d: identical rows inside a class, one unit apart across the classes" % q)
    assert not missing, "under <%d,%s> the small table lacks: %s" % (qs, "fat" if fat else "thin", "; ".join(missing))


@pytest.mark.parametrize("shape", MC.SHAPES, ids=SHAPE_IDS)
def test_chunk_cases_straddle_the_index_chunks(shape):
    qs, fat = shape
    missing = []
    cases = MC.chunk_cases()
    for c in cases:
        lay, ntv = _lay(c, shape), _ntv(c.name)
        tile, row = MC.tile_of_train(c)
        sp = MC.splits(ntv, lay)
        for b, p in c.planted.items():
            s = MC.split_of(b, lay)
            if not (b % MC.CHUNK == 0 and sp[s][0] <= b - MC.NEAR and b + MC.NEAR <= sp[s][1]):
                missing.append("%s: a split that holds the tiles %d..%d" % (c.name, b - MC.NEAR, b + MC.NEAR - 1))
            if len(p["ties"]) + len(p["runs"]) < 64:
                missing.append("%s: 64 planted queries at tile %d" % (c.name, b))
            for q, ta, tb, same in p["ties"]:
                if not (tile[ta] == b - 1 and tile[tb] == b and np.array_equal(c.d2[ta], c.d2[tb])
                        and (MC.half_of(row[ta]) == MC.half_of(row[tb])) == same):
                    missing.append("%s: query %d's identical copies in the tiles %d and %d" % (c.name, q, b - 1, b))
            if sum(same for _, _, _, same in p["ties"]) < 8:
                missing.append("%s: copies in ONE stream on both sides of tile %d" % (c.name, b))
            if sum(same and (q % (32 * qs)) // 32 == qs - 1 for q, _, _, same in p["ties"]) < 6:
                missing.append("%s: same-stream copies for queries of a wavefront's LAST set, whose chain over tile %d is pending when the "
                               "chunk ends" % (c.name, b - 1))
            for q, tr in p["runs"]:
                tt = tile[tr]
                if not ((tt < b).sum() >= 2 and (tt >= b).sum() >= 2 and tt.min() >= b - MC.NEAR and tt.max() < b + MC.NEAR):
                    missing.append("%s: query %d's run on both sides of tile %d" % (c.name, q, b))
            if not any(np.array_equal(c.d2[tr[2]], c.d2[tr[3]]) for _, tr in p["runs"]):
                missing.append("%s: an exact tie inside a run across tile %d" % (c.name, b))
        unplanted = np.setdiff1d(np.arange(len(c.d1)), MC.planted_queries(c))
        if c.d1[unplanted].max() > 89:
            missing.append("%s: unplanted queries of uniform bytes 0..89" % c.name)
        if not any(e == b0 for b0, e in sp[1:]) and not any(0 < e - b0 < lay["tiles_per_split"] for b0, e in sp):
            missing.append("%s: a short or empty last split" % c.name)
    if not any(240 in c.planted and 480 in c.planted for c in cases):
        missing.append("a size that straddles the tiles 240 and 480")
    if fat and not any(_lay(c, shape)["tiles_per_split"] % MC.STAGE_FAT == 8 for c in cases):
        missing.append("a size with tilesPerSplit % 16 == 8")
    assert not missing, "under <%d,%s> the chunk cases lack: %s" % (qs, "fat" if fat else "thin", "; ".join(missing))


def test_default_shape_of_the_chunk_cases_is_fat():
    for c in MC.chunk_cases():
        assert MC.default_shape(len(c.d1), len(c.d2)) == (2, 1), c.name


def test_big_cases_reach_what_they_are_for():
    c = MC.big_n2_case()
    assert (len(c.d2) + 255) // 256 > 256, "more pack workgroups than one pass of the scan reads"
    for shape in MC.SHAPES:
        assert 2 * _lay(c, shape)["S"] >= 200, "hundreds of streams per query"
    c = MC.many_blocks_case()
    assert len(c.d1) > 196608
    for shape in ((2, 0), (2, 1)):
        lay = _lay(c, shape)
        assert lay["nqb"] > lay["round"] and lay["S"] == 1, "more query blocks than one round of workgroups"


# ---------------- the model against the oracle; non-vacuity -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MC.SHAPES, ids=SHAPE_IDS)
def test_model_equals_oracle_on_the_small_table(oracle, shape):
    kinds, deep = set(), 0
    for c in MC.small_cases():
        S = _lay(c, shape)["S"]
        for pi in range(len(c.params)):
            got, stats = _model_rows(c, pi, S)
            _cmp(got, _oracle_rows(oracle, c, pi), "%s %r S=%d" % (c.name, c.params[pi], S))
            kinds |= {k for k, _ in stats}
            deep += sum(n >= 3 for _, n in stats)
    assert "sweep2" in kinds, "no query of the table leaves k_match_decide undecided"
    assert "reject" in kinds, "no query of the table is rejected inside k_match_decide"
    assert deep >= 1, "no query of the table makes k_match_decide recompute three groups"


@pytest.mark.parametrize("shape", MC.SHAPES, ids=SHAPE_IDS)
def test_model_equals_oracle_on_the_planted_queries_of_the_chunk_cases(oracle, shape):
    for c in MC.chunk_cases():
        S = _lay(c, shape)["S"]
        kinds = set()
        for pi in range(len(c.params)):
            got, stats = _model_rows(c, pi, S)
            _cmp(got, _oracle_rows(oracle, c, pi), "%s %r S=%d" % (c.name, c.params[pi], S))
            kinds |= {k for k, _ in stats}
        assert {"sweep2", "reject", "accept"} <= kinds, (c.name, kinds)


def test_every_case_gives_tentatives(oracle):
    """at least five for one of its parameter sets (all it can give, for a case with fewer than five queries)"""
    for c in MC.small_cases() + MC.chunk_cases():
        n = max(len(_oracle_rows(oracle, c, pi)) for pi in range(len(c.params)))
        assert n >= min(5, len(c.d1)), (c.name, n)


def test_big_cases_give_tentatives(oracle):
    """both branches of the walk at 70 000 trains give at least five; most of the 197 000 queries, near-copies of trains, give one"""
    c = MC.big_n2_case()
    for p in c.params:
        assert len(oracle.match_fginn(c.d1, c.d2, c.pos2, *p)) >= 5, (c.name, p)
    c = MC.many_blocks_case()
    for p in c.params:
        assert len(oracle.match_fginn(c.d1, c.d2, c.pos2, *p)) > len(c.d1) // 2, (c.name, p)


def test_planted_queries_end_beside_the_chunk_boundary(oracle):
    """in every chunk case at least 32 planted queries have NN0 or NNj in a tile next to the boundary"""
    for c in MC.chunk_cases():
        tile, _ = MC.tile_of_train(c)
        for b in c.planted:
            qs = set()
            for pi in range(len(c.params)):
                r = _oracle_rows(oracle, c, pi)
                near = np.isin(tile[r["t0"]], (b - 1, b)) | np.isin(tile[r["tj"]], (b - 1, b))
                qs |= set(r["q"][near].tolist())
            assert len(qs) >= 32, (c.name, b, len(qs))
