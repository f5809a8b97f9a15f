"""MatchFLANNDistance (matching/matching.cpp:607-666, linear index, HAMMING) restated in numpy, and the inputs of the Hamming tests.

Distances come from one f32 matrix product on the +-1 expansion of the bits: A B^T = (bits that agree) - (bits that differ) =
8 nbytes - 2 D, so D = (8 nbytes - A B^T) / 2 -- exact, every value and partial sum is an integer of magnitude <= 512.  The two
nearest trains are the two smallest integer keys distance * 2^22 + train index (2 000 000 < 2^22), i.e. (distance, index) in
lexicographic order.  tests/test_hamming_model_cpu.py pins this to the oracle's knn_linear on the unpacked bits, where the squared
L2 distance is the Hamming distance."""
import numpy as np

TENT = np.dtype([("q", "i4"), ("t0", "i4"), ("tj", "i4"), ("t1", "i4"), ("d1", "f8"), ("d2", "f8"),
                 ("d2by2ndcl", "f8"), ("ratio", "f8")], align=True)
CHUNK = 1024      # queries per matrix product


def pm1(b):
    b = np.ascontiguousarray(b, np.uint8)
    return np.unpackbits(b, axis=1).astype(np.float32) * 2 - 1


def distances(b1, b2):
    """[n1][n2] int32 Hamming distances of two [n][nbytes] u8 arrays"""
    nbits = 8 * b1.shape[1]
    return ((nbits - pm1(b1) @ pm1(b2).T) / 2).astype(np.int32)


def knn2(b1, b2):
    """[n1][4] int32 = first, d(first), second, d(second); needs n2 >= 2"""
    b1, b2 = np.ascontiguousarray(b1, np.uint8), np.ascontiguousarray(b2, np.uint8)
    n1, n2 = len(b1), len(b2)
    assert n2 >= 2 and b1.shape[1] == b2.shape[1]
    B = pm1(b2).T.copy()
    nbits = 8 * b1.shape[1]
    idx = np.arange(n2, dtype=np.int64)
    out = np.zeros((n1, 4), np.int32)
    for lo in range(0, n1, CHUNK):
        D = ((nbits - pm1(b1[lo:lo + CHUNK]) @ B) / 2).astype(np.int64)
        key = D * (1 << 22) + idx
        two = np.sort(np.partition(key, 1, axis=1)[:, :2], axis=1)
        out[lo:lo + CHUNK, 0] = two[:, 0] & ((1 << 22) - 1)
        out[lo:lo + CHUNK, 1] = two[:, 0] >> 22
        out[lo:lo + CHUNK, 2] = two[:, 1] & ((1 << 22) - 1)
        out[lo:lo + CHUNK, 3] = two[:, 1] >> 22
    return out


def tentatives(nn2, distance_threshold):
    """the record rule, matching.cpp:610, 647-661"""
    nn2 = np.asarray(nn2, np.int32).reshape(-1, 4)
    max_distance = int(np.float32(distance_threshold))
    q = np.nonzero(nn2[:, 1] <= max_distance)[0]
    t = np.zeros(len(q), TENT)
    t["q"], t["t0"], t["tj"], t["t1"] = q, nn2[q, 0], nn2[q, 2], nn2[q, 2]
    t["d1"], t["d2"], t["d2by2ndcl"] = nn2[q, 1], nn2[q, 3], nn2[q, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t["ratio"] = t["d1"] / t["d2"]
    return t


def match(b1, b2, distance_threshold):
    if len(b1) == 0 or len(b2) == 0:
        return np.zeros(0, TENT)
    return tentatives(knn2(b1, b2), distance_threshold)


def same_tents(got, ref):
    assert len(got) == len(ref), (len(got), len(ref))
    for f in TENT.names:
        assert np.array_equal(got[f], ref[f], equal_nan=(f == "ratio")), f


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def binarise(d):
    """[n][128] real descriptors -> [n][16] u8: bit j = d[j] > median of the row"""
    d = np.asarray(d, np.float32)
    return np.packbits(d > np.median(d, axis=1, keepdims=True), axis=1)


def random_rows(n1, n2, nbytes, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (n1, nbytes)).astype(np.uint8), rs.randint(0, 256, (n2, nbytes)).astype(np.uint8)


def tie_heavy():
    """70 x 257 rows of 4 bytes drawn from {0x00, 0x0F, 0xFF}; the second half of the trains is a copy of the first"""
    rs = np.random.RandomState(5)
    v = np.array([0x00, 0x0F, 0xFF], np.uint8)
    q = v[rs.randint(0, 3, (70, 4))]
    t = v[rs.randint(0, 3, (257, 4))]
    t[129:] = t[:128]
    return q, t


def flip(row, bits):
    r = np.unpackbits(row.copy())
    r[np.asarray(bits, int)] ^= 1
    return np.packbits(r)


PLANT = dict(nan=0, at_max=1, above_max=2, tie_first=3, tie_second=4, copies=5)   # query index of every planted case
MAX_DISTANCE = 60


def planted(n1, n2, nbytes, copies_at, seed=11):
    """Queries that are noisy copies of trains (k bit flips, k spread over 0..70, far below the ~100 of the nearest unrelated row
    at >= 16 bytes), with these rows planted (PLANT):
      nan         two exact copies of the query among the trains: d1 = d2 = 0, ratio NaN
      at_max      nearest train at exactly MAX_DISTANCE;  above_max: at MAX_DISTANCE + 1
      tie_first   two trains at the same smallest distance;  tie_second: two trains tie for the second neighbour
      copies      the query's nearest train (distance 2) stands at every index of copies_at
    Needs nbytes >= 16, n1 >= 8, n2 >= 16 and copies_at disjoint from the indices used below."""
    rs = np.random.RandomState(seed)
    nbits = 8 * nbytes
    t = rs.randint(0, 256, (n2, nbytes)).astype(np.uint8)
    src = rs.randint(0, n2, n1)
    q = np.stack([flip(t[src[i]], rs.choice(nbits, rs.randint(0, 71), replace=False)) for i in range(n1)])
    q[:len(PLANT)] = rs.randint(0, 256, (len(PLANT), nbytes))      # the planted queries are related to their planted trains only
    free = [i for i in range(n2) if i not in set(int(c) for c in copies_at)]
    a = free[3:13]      # ten train slots for the plants, low indices but not 0
    t[a[0]] = q[PLANT["nan"]]; t[a[1]] = q[PLANT["nan"]]
    t[a[2]] = flip(q[PLANT["at_max"]], np.arange(MAX_DISTANCE))
    t[a[3]] = flip(q[PLANT["above_max"]], np.arange(MAX_DISTANCE + 1))
    t[a[4]] = flip(q[PLANT["tie_first"]], [0, 9, 18, 27, 36]); t[a[5]] = flip(q[PLANT["tie_first"]], [1, 10, 19, 28, 37])
    t[a[6]] = flip(q[PLANT["tie_second"]], [3, 4, 5])
    t[a[7]] = flip(q[PLANT["tie_second"]], np.arange(40, 49)); t[a[8]] = flip(q[PLANT["tie_second"]], np.arange(60, 69))
    near = flip(q[PLANT["copies"]], [7, 77])
    for c in copies_at:
        t[int(c)] = near
    return q, t, dict(nan=(a[0], a[1]), at_max=a[2], above_max=a[3], tie_first=(a[4], a[5]), tie_second=(a[6], a[7], a[8]),
                      copies=sorted(int(c) for c in copies_at))


def check_planted(nn2, info):
    """the planted rows come out as planted() says (model or device result)"""
    P = PLANT
    assert tuple(nn2[P["nan"]]) == (info["nan"][0], 0, info["nan"][1], 0)
    assert tuple(nn2[P["at_max"]][:2]) == (info["at_max"], MAX_DISTANCE)
    assert tuple(nn2[P["above_max"]][:2]) == (info["above_max"], MAX_DISTANCE + 1)
    assert tuple(nn2[P["tie_first"]]) == (info["tie_first"][0], 5, info["tie_first"][1], 5)
    assert tuple(nn2[P["tie_second"]]) == (info["tie_second"][0], 3, info["tie_second"][1], 9)
    assert tuple(nn2[P["copies"]]) == (info["copies"][0], 2, info["copies"][1], 2)


def copies_for(T, start):
    """index 0, the last index of the first tile, the first index of the last split"""
    return [0, T - 1, start]


def last_split_start(T, n2, splits_used):
    ntiles = (n2 + T - 1) // T
    tps = (ntiles + splits_used - 1) // splits_used
    return (splits_used - 1) * tps * T
