"""Executable model (numpy) of MatchFlannFGINNPlusDB (matching/matching.cpp:462-572) over an exact (linear) search.

Test infrastructure: `tests/test_fginn_db_model_cpu.py` pins it to the oracle's MatchFlannFGINN restatement on the CPU;
`tests/test_gpu_fginn_db.py` compares the device matcher (`modsx_match_fginn_db`, the fused callers with a database attached)
against it, record for record.

  match_fginn_db   the reference's two loops as they stand: distances in f32 by sgemm (exact: the descriptors hold the integers
                   0..255, every partial sum is an integer below 2^24), neighbours ordered by (distance, train index), the walk of
                   both branches with `max` = std::max (a < b ? b : a, so a NaN ratioDB is ignored) and d2byDB.
  filter_plain     the formulation the device uses: ratioDB does not depend on j, so the records are the plain FGINN records,
                   filtered (kept iff ratioDB is NaN or <= ratio^2) and relabelled (ratio = sqrt(max(r_j, ratioDB))).
  planted_input    the real-descriptor input of the tests: queries / trains of a small pair, a database of unrelated descriptors
                   plus jittered copies of every second train, one query planted in a train AND the database (ratioDB = 0/0), one
                   planted in the database only (ratioDB = +inf).
"""
import numpy as np

TENT = np.dtype([("q", "i4"), ("t0", "i4"), ("tj", "i4"), ("t1", "i4"), ("d1", "f8"), ("d2", "f8"),
                 ("d2by2ndcl", "f8"), ("ratio", "f8")], align=True)


def sqdist_f32(a, b):
    """[len(a), len(b)] squared L2 distances in float32 (|a|^2 + |b|^2 - 2 a.b by sgemm): exact on integers 0..255"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    na = (a * a).sum(1, dtype=np.float32)[:, None]
    nb = (b * b).sum(1, dtype=np.float32)[None, :]
    return (na + nb) - np.float32(2.0) * (a @ b.T)


def db_nearest(d1, db, chunk=1 << 15):
    """squared distance of every query to its nearest database row, float32 (chunked over the database)"""
    best = np.full(len(d1), np.inf, np.float32)
    for s in range(0, len(db), chunk):
        best = np.minimum(best, sqdist_f32(d1, db[s:s + chunk]).min(1))
    return best


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(np.float32(a) / np.float32(b))      # `double ratio = distsRow[0]/distsRow[j]`: f32 division, widened


def match_fginn_db(d1, d2, pos2, db, ratio=0.8, contrad=30.0, nn=50, ddb=None):
    """(records, d2byDB).  db = None (and ddb = None): plain MatchFlannFGINN (:357-461), d2byDB empty."""
    sq, cd = ratio * ratio, contrad * contrad
    n1, n2 = len(d1), len(d2)
    out, d2db = [], []
    if n1 == 0 or n2 == 0:
        return np.zeros(0, TENT), np.zeros(0)
    if ddb is None and db is not None:
        ddb = db_nearest(d1, db)
    D = sqdist_f32(d1, d2)
    pos2 = np.asarray(pos2, np.float64)
    k = min(nn, n2)
    for i in range(n1):
        idx = np.argsort(D[i], kind="stable")[:k]          # ties by ascending train index
        ds = D[i][idx]
        rdb = _div(ds[0], ddb[i]) if ddb is not None else None
        for j in range(1, nn):
            if j >= k:
                break                                      # fewer than nn trains: the walk runs off the list
            r = _div(ds[0], ds[j])
            dx, dy = pos2[idx[0]] - pos2[idx[j]]
            far = dx * dx + dy * dy > cd
            if sq >= 1.0:                                  # "to get all points" (:505-536)
                take = j == nn - 1 or far
            else:
                if rdb is not None and r < rdb:            # std::max(ratio, ratioDB) (:548)
                    r = rdb
                take = r <= sq                             # NaN fails
            if take:
                out.append((i, idx[0], idx[j], idx[1], ds[0], ds[j], ds[1], np.sqrt(r)))
                if ddb is not None:
                    d2db.append(np.float64(ddb[i]))
                break
            if sq < 1.0 and far:
                break                                      # first contradictive (:568)
    return np.array(out, TENT) if out else np.zeros(0, TENT), np.array(d2db, np.float64)


def filter_plain(plain, ddb, ratio):
    """the plain FGINN records -> the database variant's records (the host half of the device matcher)"""
    sq = ratio * ratio
    keep, rat, d2db = [], [], []
    for t in plain:
        dq = ddb[t["q"]]
        r = _div(t["d1"], t["d2"])
        if sq < 1.0:
            rdb = _div(t["d1"], dq)
            if r < rdb:
                r = rdb
            if not r <= sq:
                continue
        keep.append(t)
        rat.append(np.sqrt(r))
        d2db.append(np.float64(dq))
    out = np.array(keep, TENT) if keep else np.zeros(0, TENT)
    if len(out):
        out["ratio"] = rat
    return out, np.array(d2db, np.float64)


def same_tents(a, b):
    """field-wise exact equality (as tests/test_gpu_parity.py _check_tents); a NaN `ratio` -- 0/0 in the all-points branch, which
    has no ratio test -- equals a NaN"""
    assert len(a) == len(b), (len(a), len(b))
    for f in TENT.names:
        assert np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f"), f


def background_descriptors(oracle, seeds=(11, 12)):
    """oracle RootSIFT descriptors of synthetic images that have nothing to do with the test pair"""
    from common import oracle_features
    from mods_amd import synthetic
    out = []
    for s in seeds:
        a, b, _ = synthetic.make_pair(rows=240, cols=320, nblobs=420, seed=s)
        out.append(oracle_features(oracle, a)[2])
        out.append(oracle_features(oracle, b)[2])
    return np.concatenate(out).astype(np.float32)


def planted_input(oracle, small_pair, seed=5):
    """dict(d1, d2, pos2, db, q_nan, q_inf): see the module docstring"""
    from common import oracle_features
    a, b, _ = small_pair
    _, _, d1 = oracle_features(oracle, a)
    _, r2, d2 = oracle_features(oracle, b)
    d1, d2 = d1.astype(np.float32).copy(), d2.astype(np.float32).copy()
    pos2 = np.stack([r2["reproj_kp"]["x"], r2["reproj_kp"]["y"]], 1)
    rs = np.random.RandomState(seed)
    jit = np.clip(d2[::2] + rs.randint(-3, 4, d2[::2].shape), 0, 255).astype(np.float32)
    plain, _ = match_fginn_db(d1, d2, pos2, None, 0.8, 30.0)
    # +inf: a query that HAS a plain record and does not sit on its nearest train, copied into the database only
    q_inf = int(plain["q"][plain["d1"] > 0][0])
    # NaN: another query copied into a train (far from its own nearest one in the list) and into the database
    q_nan = int([q for q in plain["q"] if q != q_inf][1])
    t_nan = int(plain["t0"][plain["q"] == q_nan][0])
    d2[t_nan] = d1[q_nan]
    db = np.concatenate([background_descriptors(oracle), jit, d1[q_nan][None], d1[q_inf][None]]).astype(np.float32)
    return dict(d1=d1, d2=d2, pos2=pos2, db=db, q_nan=q_nan, q_inf=q_inf)
