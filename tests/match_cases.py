"""Deterministic inputs for the matcher tests, and a restatement of the launcher's geometry (kernels_match.hip match_layout).

A helper, not a test module.  Every case is a `Case`: (d1, d2, pos2, [(ratio, contrad, nn), ...]) followed by its name and, for the
chunk cases, what was planted where.  Descriptors are float32 arrays holding the integers 0..255; the arrays are read-only and
cached, so every test of a run sees the same objects.

The restated layout (`layout`, `splits`) is used to ASSERT COVERAGE only -- which case reaches which path under which of the four
shapes of k_match_sweep1<QS, FAT> -- never to produce expected values: those come from the oracle.  tests/test_gpu_match_shapes.py
compares it with what the launcher really used (mods_amd.last_match_geometry()).

Planted trains are placed by PACKED SLOT: `tests.match_model.pack(d2)` says which virtual tile (even class first, then odd) and
which row a train lands in; a planted row takes the parity of the train it replaces, so the packing does not move.
"""
import collections
import functools

import numpy as np

from tests.match_model import pack

TPS, MINT, CHUNK = 4, 12, 240          # match_core.hpp: tiles per stage, fewest tiles of a split, tiles per index chunk
STAGE_FAT = 16                         # tiles a fat workgroup stages per barrier (s1_spb(true) * TPS)
SHAPES = ((2, 0), (2, 1), (4, 0), (4, 1))       # (QS, FAT) of k_match_sweep1

Case = collections.namedtuple("Case", "d1 d2 pos2 params name planted")
Case.__new__.__defaults__ = (None,)


# ---------------- the launcher's geometry, restated ---------------------------------------------------------------------------
def sweep_wps(qs):
    return 2 if qs >= 4 else 3


def s1_qpb(qs, fat):
    """queries of one workgroup of sweep 1"""
    return (4 * sweep_wps(qs) if fat else 4) * 32 * qs


def s1_round(qs, fat):
    """workgroups of one round"""
    return 256 if fat else 256 * sweep_wps(qs)


def ntiles_ub(n2):
    return ((n2 + 31) // 32 + TPS - 1) // TPS * TPS + 2 * TPS


def default_shape(n1, n2, nb=1):
    """(QS, FAT) the launcher picks when neither MODSX_MATCH_QSETS nor MODSX_SWEEP1_FAT is set and one context is busy"""
    return (4 if nb == 1 and n1 >= 40000 and n2 >= 40000 else 2), int(n1 >= 16000)


def layout(n1, n2, qs, fat):
    qpb = s1_qpb(qs, fat)
    nqb = (n1 + qpb - 1) // qpb
    nt = ntiles_ub(n2)
    S = max(1, min(s1_round(qs, fat) // nqb, nt // MINT))
    tps = ((nt + S - 1) // S + TPS - 1) // TPS * TPS
    S = max(1, (nt + tps - 1) // tps)
    return dict(qs=qs, fat=int(fat), S=S, tiles_per_split=tps, ntiles_ub=nt, qpb=qpb, nqb=nqb, round=s1_round(qs, fat))


def splits(ntiles_v, lay):
    """[tBeg, tEnd) of every split over the virtual tiles the device counts (k_match_pack's ntilesV); the last ones may be short or empty"""
    tps = lay["tiles_per_split"]
    return [(s * tps, max(s * tps, min((s + 1) * tps, ntiles_v))) for s in range(lay["S"])]


def split_of(tile, lay):
    return tile // lay["tiles_per_split"]


def half_of(row):
    """lane half of the sweeps that owns a tile row (inverse of row_of)"""
    return (row >> 2) & 1


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def near_duplicates(rs, row, k, lo=-2, hi=3, floor=0):
    """k rows within `lo`..`hi - 1` of `row` in every element (the planted runs of the parity tests and of tools/fuzz_match.py)"""
    return np.clip(row[None, :] + rs.randint(lo, hi, (k, 128)), floor, 255)


def same_tentatives(a, b):
    """every field equal (NaN == NaN for the ratio of 0 / 0)"""
    if len(a) != len(b):
        return False
    for f in a.dtype.names:
        if not np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f"):
            return False
    return True


# ---------------- the three adversarial generators of tests/test_gpu_parity.py ------------------------------------------------
@functools.lru_cache(None)
def tie_cases():
    """low-entropy descriptors: many exact distance ties, duplicated trains, zero distances; one tile to nine, ragged"""
    rs = np.random.RandomState(9)
    out = []
    for n1, n2 in ((1, 50), (33, 95), (70, 257), (5, 64)):
        d1 = rs.randint(0, 3, (n1, 128)).astype(np.float32) * 40
        d2 = rs.randint(0, 3, (n2, 128)).astype(np.float32) * 40
        d2[n2 // 2:] = d2[: n2 - n2 // 2]                       # duplicated trains
        d1[0] = d2[3]                                          # exact hit (d0 = 0)
        pos2 = rs.uniform(0, 60, (n2, 2))                      # dense positions: long walks through consistent NNs
        out.append(Case(*_ro(d1, d2, pos2), ((0.8, 30.0, 50), (0.95, 80.0, 50), (0.8, 5.0, 50)), "ties_%dx%d" % (n1, n2)))
    return tuple(out)


@functools.lru_cache(None)
def all_points_case():
    """ratio >= 1: runs of near-duplicates at one place whose walks go down to rank nn - 1, and an exact tie"""
    rs = np.random.RandomState(5)
    n1, n2 = 300, 3000
    e2 = rs.randint(1, 90, (n2, 128)).astype(np.float32)
    e1 = rs.randint(1, 90, (n1, 128)).astype(np.float32)
    p2 = rs.uniform(0, 300, (n2, 2))
    for q in range(0, n1, 2):
        k = int(rs.randint(2, 60))
        start = int(rs.randint(0, n2 - k))
        e2[start:start + k] = np.clip(e1[q][None, :] + rs.randint(-2, 3, (k, 128)), 1, 255)
        p2[start:start + k] = p2[start] + rs.uniform(-3, 3, (k, 2))
    e2[7] = e2[8]                                                   # an exact tie
    return Case(*_ro(e1, e2, p2), ((1.0, 30.0, 50), (1.5, 10.0, 8), (1.0, 500.0, 100)), "all_points_300x3000")


@functools.lru_cache(None)
def clustered_cases():
    """runs of up to 40 (150) near-duplicate trains of one query in one stream, 20 event groups in one stream, ties inside runs"""
    rs = np.random.RandomState(31)
    out = []
    for n1, n2, kmax in ((300, 2100, 40), (40, 5000, 25), (513, 1000, 12), (60, 3000, 150)):   # (the last: runs beyond 64, for nn > 64)
        base = rs.randint(0, 90, (n2, 128)).astype(np.float32)
        d2 = base.copy()
        d1 = rs.randint(0, 90, (n1, 128)).astype(np.float32)
        pos2 = rs.uniform(0, 2000, (n2, 2))
        for q in range(0, n1, 3):
            k = int(rs.randint(2, kmax))
            start = int(rs.randint(0, n2 - k))
            near = np.clip(d1[q][None, :] + rs.randint(-2, 3, (k, 128)), 0, 255)
            d2[start:start + k] = near                     # contiguous: same tiles, same stream
            pos2[start:start + k] = pos2[start] + rs.uniform(-3, 3, (k, 2))
            if q % 6 == 0:
                d2[start + k - 1] = d2[start]               # an exact tie inside the run
        # one near-duplicate per tile, always in the same lane half, over 20 consecutive tiles of the first split: 20 event
        # groups in ONE stream (> 16 slots) but fewer than nn in total -> the stream is rescanned exactly
        for q in (1, 4, 7):
            t0 = 32 * (q % 3)
            for j in range(20):
                t = t0 + 32 * j + 1
                if t < n2:
                    d2[t] = np.clip(d1[q] + rs.randint(-2, 3, 128), 0, 255)
                    pos2[t] = pos2[t0 + 1] + rs.uniform(-3, 3, 2)
        params = ((0.8, 30.0, 50), (0.9, 30.0, 20), (0.8, 2.0, 50), (0.9, 30.0, 100), (0.95, 40.0, 256), (0.9, 30.0, 65))
        out.append(Case(*_ro(d1, d2, pos2), params, "clustered_%dx%d" % (n1, n2)))
    return tuple(out)


# ---------------- parity classes ----------------------------------------------------------------------------------------------
def _set_parity(rows, par):
    """flip the lowest bit of the last element where a row's parity differs from `par` (values stay in 0..255)"""
    rows = rows.astype(np.int64)
    flip = (rows.sum(1) & 1) != par
    rows[flip, 127] ^= 1
    return rows


@functools.lru_cache(None)
def odd_only_case():
    """every train has odd sum(b): the even class is empty (TEp = 0, the virtual sequence starts in the odd region).  The tie
    alphabet of tie_cases() with the parity forced; 261 queries = one 256-query block and five"""
    rs = np.random.RandomState(41)
    n1, n2 = 261, 700
    d1 = rs.randint(0, 3, (n1, 128)) * 40
    d2 = _set_parity(rs.randint(0, 3, (n2, 128)) * 40, 1)
    d2[n2 // 2:] = d2[: n2 - n2 // 2]
    pos2 = rs.uniform(0, 60, (n2, 2))
    for q in range(0, n1, 4):                                   # near-duplicates (odd as well) so that ratios pass
        k = int(rs.randint(1, 5))
        at = rs.choice(n2, k, replace=False)
        d2[at] = _set_parity(near_duplicates(rs, d1[q], k), 1)
        pos2[at] = pos2[at[0]] + rs.uniform(-3, 3, (k, 2))
    d1[0] = d2[3]
    assert ((d2.sum(1) & 1) == 1).all()
    return Case(*_ro(d1.astype(np.float32), d2.astype(np.float32), pos2), ((0.8, 30.0, 50), (0.95, 80.0, 50), (0.8, 5.0, 12)),
                "odd_only_261x700")


@functools.lru_cache(None)
def class_boundary_case():
    """Half even, half odd trains (alternating), 640 of each: 20 full tiles per class, so virtual tile 19 is the last even tile and
    20 = TEp the first odd one, with no padding between.  Equal distances cannot cross the classes (the parity of a distance to a
    query is the parity of the train), so a planted run is: copies of ONE even row R as the last even trains -- exact ties in tile
    19 -- and copies of R' = R with one element one higher as the first odd trains -- exact ties in tile 20, one unit of a
    coordinate away from the first half of the run.  517 queries = one 512-query block and five."""
    rs = np.random.RandomState(43)
    n1, n2 = 517, 1280
    d1 = rs.randint(0, 90, (n1, 128))
    d2 = _set_parity(rs.randint(0, 90, (n2, 128)), np.arange(n2) & 1)
    pos2 = rs.uniform(0, 2000, (n2, 2))
    planted = []
    nq, m = 10, 3                                               # 10 queries x (3 even + 3 odd) trains
    qs = np.linspace(0, n1 - 1, nq).astype(int)
    for i, q in enumerate(qs):
        R = near_duplicates(rs, d1[q], 1)
        R[0, 5] = min(R[0, 5], 254)
        R = _set_parity(R, 0)[0]
        R2 = R.copy()
        R2[5] += 1
        ev = n2 - 2 - 2 * (i * m + np.arange(m))                # the last even trains
        od = 1 + 2 * (i * m + np.arange(m))                     # the first odd trains
        d2[ev] = R
        d2[od] = R2
        centre = rs.uniform(0, 2000, 2)
        pos2[np.r_[ev, od]] = centre + rs.uniform(-3, 3, (2 * m, 2)) if i % 3 else rs.uniform(0, 2000, (2 * m, 2))
        planted.append((int(q), sorted(int(t) for t in ev), sorted(int(t) for t in od)))
    assert ((d2.sum(1) & 1) == (np.arange(n2) & 1)).all()
    return Case(*_ro(d1.astype(np.float32), d2.astype(np.float32), pos2), ((0.8, 30.0, 50), (0.9, 30.0, 5), (0.8, 2.0, 50)),
                "class_boundary_517x1280", dict(runs=planted))


@functools.lru_cache(None)
def ragged_block_cases():
    """773 and 1029 queries: one block of the fat shapes (768 / 1024 queries) and five; scattered near-duplicates"""
    out = []
    for n1, seed in ((773, 47), (1029, 53)):
        rs = np.random.RandomState(seed)
        n2 = 700
        d1 = rs.randint(0, 90, (n1, 128))
        d2 = rs.randint(0, 90, (n2, 128))
        pos2 = rs.uniform(0, 2000, (n2, 2))
        free = rs.permutation(n2)
        at = 0
        for q in list(range(0, n1, 11)) + list(range(n1 - 5, n1)):
            k = int(rs.randint(1, 7))
            if at + k > n2:
                break
            t = free[at:at + k]
            at += k
            d2[t] = near_duplicates(rs, d1[q], k)
            pos2[t] = pos2[t[0]] + (rs.uniform(-3, 3, (k, 2)) if q % 5 else rs.uniform(-300, 300, (k, 2)))
            if k > 2 and q % 2:
                d2[t[-1]] = d2[t[0]]
        out.append(Case(*_ro(d1.astype(np.float32), d2.astype(np.float32), pos2), ((0.8, 30.0, 50), (0.9, 30.0, 4)),
                        "ragged_%dx%d" % (n1, n2), dict(queries=list(range(0, n1, 11)))))
    return tuple(out)


def small_cases():
    """one table for every shape"""
    return tie_cases() + (all_points_case(),) + clustered_cases() + (odd_only_case(), class_boundary_case()) + ragged_block_cases()


# ---------------- index chunks ------------------------------------------------------------------------------------------------
NEAR = 4          # planted trains sit in the tiles b - NEAR .. b + NEAR - 1 around a chunk boundary b: whole stages, so every split
#                   that straddles b holds all of them, whatever its length


def _chunk_case(name, n1, n2, n_even, seed, boundaries, params):
    """Uniform bytes 0..89 everywhere, the parity of random trains flipped until `n_even` of them are even (that fixes which class
    the tiles around a boundary belong to); around every chunk boundary b (a multiple of CHUNK), for 64 queries of its own:
      ties  32 queries: two IDENTICAL near-duplicates of the query, one in tile b - 1 (the chain that is still pending when the chunk
            ends) and one in tile b.  For 16 of them both copies sit in the same lane half: one stream holds the copy as its best key
            before the flush and meets an equal key after it; for the other 16 the halves differ.  The oracle returns the lower
            train as NN0 and the higher one as NN1.  Eight of the same-half queries sit in the last query set of their wavefront, whose
            chain over tile b - 1 is drained at the chunk end.
      runs  32 queries: six near-duplicates, one in each of the tiles b - 4, b - 3, b - 2, b + 1, b + 2, b + 3 -- six groups, more than
            k_match_decide recomputes; every fourth run is scattered over the image (a contradictive neighbour), every eighth has
            an exact tie across the boundary (tiles b - 2 and b + 1).
    The eight tiles hold planted trains only."""
    rs = np.random.RandomState(seed)
    d1 = rs.randint(0, 90, (n1, 128))
    d2 = _set_parity(rs.randint(0, 90, (n2, 128)), (rs.permutation(n2) >= n_even).astype(np.int64))
    pos2 = rs.uniform(0, 2000, (n2, 2))
    perm, tpar = pack(d2)
    queries = rs.permutation(np.linspace(0, n1 - 1, 64 * len(boundaries)).astype(int))     # first and last block included
    # The chain still PENDING when tile b - 1 ends a chunk is that of a wavefront's last query set (set QS - 1 of its 32 QS queries):
    # every other same-half tie query of a boundary is moved, inside its block of 128 queries, to the last 32 of it -- the last set
    # under QS = 4 and under QS = 2 alike.
    taken = set(queries.tolist())
    for bi in range(len(boundaries)):
        for i in range(0, 16, 2):
            q = int(queries[64 * bi + i])
            moved = q // 128 * 128 + 96 + q % 32
            if moved < n1 and moved not in taken:
                taken.discard(q)
                taken.add(moved)
                queries[64 * bi + i] = moved
    assert len(set(queries.tolist())) == len(queries)
    planted = {}
    for bi, b in enumerate(boundaries):
        tiles = list(range(b - NEAR, b + NEAR))
        assert b + NEAR <= len(tpar) and len(set(tpar[tiles])) == 1 and (perm[(b - NEAR) * 32:(b + NEAR) * 32] >= 0).all(), \
            "%s: the tiles around %d are not real tiles of one class" % (name, b)
        par = int(tpar[b])
        qs = queries[64 * bi:64 * bi + 64]
        rows = {t: [list(rs.permutation([r for r in range(32) if half_of(r) == h])) for h in (0, 1)] for t in tiles}

        def put(tile, half, vec, xy):
            if half is None:
                half = int(len(rows[tile][1]) > len(rows[tile][0]))
            t = int(perm[tile * 32 + rows[tile][half].pop()])
            d2[t] = vec
            pos2[t] = xy
            return t
        ties, runs = [], []
        for i, q in enumerate(qs[:32]):
            R = _set_parity(near_duplicates(rs, d1[q], 1), par)[0]
            h1 = (i >> 3) & 1                                   # i < 16: the same half; then different halves
            h2 = h1 if i < 16 else 1 - h1
            xy = rs.uniform(0, 2000, 2)
            ta = put(b - 1, h1, R, xy + rs.uniform(-3, 3, 2))
            tb = put(b, h2, R, xy + rs.uniform(-3, 3, 2))
            ties.append((int(q), ta, tb, i < 16))
        for i, q in enumerate(qs[32:]):
            near = _set_parity(near_duplicates(rs, d1[q], 6), par)
            if i % 8 == 0:
                near[3] = near[2]                               # tiles b - 2 and b + 1
            xy = rs.uniform(0, 2000, 2)
            tr = []
            for j, tile in enumerate((b - 4, b - 3, b - 2, b + 1, b + 2, b + 3)):
                tr.append(put(tile, None, near[j], rs.uniform(0, 2000, 2) if i % 4 == 3 else xy + rs.uniform(-3, 3, 2)))
            runs.append((int(q), tr))
        assert all(not rows[t][0] and not rows[t][1] for t in tiles)
        planted[b] = dict(ties=ties, runs=runs)
    perm2, _ = pack(d2)
    assert np.array_equal(perm, perm2), "planting moved the packing"
    return Case(*_ro(d1.astype(np.float32), d2.astype(np.float32), pos2), params, name, planted)


# Sizes from the restated layout (tests/test_match_cases_cpu.py asserts what is claimed here), tilesPerSplit under
# <2,thin> <2,fat> <4,thin> <4,fat>:
#   20000 x  9000   36 36 28 28   none divides 240                  (the smallest n2 with that property at 20 k queries)
#   20000 x 15800   56 56 44 44   none divides 240 or 480; 56 = 8 mod 16 for <2,fat>
#   26500 x 15800   72 72 56 56   none divides 240 or 480; 56 = 8 mod 16 for <4,fat>
@functools.lru_cache(None)
def chunk_cases():
    return (_chunk_case("chunk_20000x9000", 20000, 9000, 4500, 61, (240,), ((0.8, 30.0, 50), (0.9, 30.0, 6))),
            _chunk_case("chunk_20000x15800", 20000, 15800, 7936, 67, (240, 480), ((0.8, 30.0, 50), (0.9, 30.0, 6))),
            _chunk_case("chunk_26500x15800", 26500, 15800, 7936, 71, (240, 480), ((0.8, 30.0, 50),)))


def planted_queries(case):
    """queries of a chunk case that something was planted for, ascending"""
    return np.array(sorted(q for p in case.planted.values() for q in [t[0] for t in p["ties"]] + [r[0] for r in p["runs"]]))


def model_queries(case):
    """the queries tests/test_match_cases_cpu.py runs through the numpy model (it is per query and slow): every query of a small
    problem; of a larger one the planted queries, 64 spread over the rest and the last five"""
    n1 = len(case.d1)
    if n1 <= 128:
        return np.arange(n1)
    if case.planted and "ties" in next(iter(case.planted.values()), ()):
        return planted_queries(case)
    extra = []
    if case.planted:
        extra = case.planted.get("queries", []) + [r[0] for r in case.planted.get("runs", [])]
    return np.unique(np.r_[np.array(extra, int), np.linspace(0, n1 - 1, 64).astype(int), np.arange(n1 - 5, n1)])


# ---------------- big sizes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def big_n2_case():
    """70 000 trains: 274 workgroups of k_match_pack (more than the 256 slots of a waiting workgroup's miss list, more than the 256
    threads that read the status words in one pass), 183 splits -> 366 streams per query in k_match_decide; both branches of the walk"""
    rs = np.random.RandomState(4)
    n1, n2 = 96, 70000
    d2 = rs.randint(0, 120, (n2, 128)).astype(np.float32)
    d1 = np.clip(d2[rs.choice(n2, n1)] + rs.randint(-3, 4, (n1, 128)), 0, 255).astype(np.float32)
    pos2 = rs.uniform(0, 2000, (n2, 2))
    return Case(*_ro(d1, d2, pos2), ((0.8, 30.0, 50), (1.0, 30.0, 50)), "big_n2_96x70000")


@functools.lru_cache(None)
def many_blocks_case():
    """197 000 queries: more query blocks than one round of workgroups under both QS = 2 shapes (770 > 768 thin, 257 > 256 fat: S
    computed as 0 and clamped to 1).  Queries are near-copies of random trains, so most of them give a tentative."""
    rs = np.random.RandomState(73)
    n1, n2 = 197000, 384
    d2 = rs.randint(0, 90, (n2, 128))
    src = rs.randint(0, n2, n1)
    d1 = np.clip(d2[src] + rs.randint(-2, 3, (n1, 128), dtype=np.int8), 0, 255)
    pos2 = rs.uniform(0, 2000, (n2, 2))
    return Case(*_ro(d1.astype(np.float32), d2.astype(np.float32), pos2), ((0.8, 30.0, 8),), "many_blocks_197000x384")


def big_cases():
    return (big_n2_case(), many_blocks_case())


def ntiles_v(case):
    """virtual tiles the device counts for the case (both classes padded to whole stages)"""
    return len(pack(case.d2)[1])


def tile_of_train(case):
    """train index -> (virtual tile, row)"""
    perm, _ = pack(case.d2)
    slot = np.full(len(case.d2), -1, np.int64)
    slot[perm[perm >= 0]] = np.nonzero(perm >= 0)[0]
    return slot >> 5, slot & 31
