"""CPU: the refill rule of the queue-fed Baumberg kernel (variant 3; tests/baumberg_queue_model.py restates it in numpy) over the
1 295 jobs of tests/baumberg_cases.py with the oracle's iteration counts.  tests/test_gpu_baumberg_queue.py runs the kernel on the
same lists; this module shows without a device what the rule does with them.

  1. every job is handed out exactly once, at 1, 2, 3, 8 and 400 wavefronts per range, and no counter passes the length of its
     range by more than wavefronts x K (a wavefront overshoots a counter once at most: it never asks an empty range again)
  2. a round with an idle slot happens only once all eight ranges are exhausted
  3. the launch runs no more rounds than the static chunks at the production chunk of the same n (BC.schedule), wherever there is
     something to refill from: 1, 2, 3 and 8 wavefronts per range, i.e. at least 20 jobs per wavefront.  At 400 per range there are
     more slots than jobs, no slot is ever refilled and the queue is the static schedule at chunk 2 with another pairing (its
     ranges start on odd jobs), for which no inequality holds either way; production never launches more than ceil(n / K)
     wavefronts.  What holds there instead is asserted: no wavefront runs more than K jobs, its rounds are those of its longest
     job, and the launch is as long as the longest job.
  4. stealing happens on the list as it is (the ranges are not equally heavy), and on a front-loaded list -- every iteration-limit
     job in the first range -- wavefronts of all seven other ranges take from the first
"""
import numpy as np
import pytest

from tests import baumberg_cases as BC
from tests import baumberg_queue_model as QM

K = 2
WAVES_PER_RANGE = (1, 2, 3, 8, 400)


@pytest.fixture(scope="module")
def res(oracle):
    return BC.oracle_results(oracle)


@pytest.fixture(scope="module")
def lists(res):
    """name -> passes of the list: the case list as it is, and the front-loaded one"""
    p = BC.passes_of(res)
    return {"cases": p, "front-loaded": p[QM.front_loaded_order(res["reason"])]}


_sims = {}


def _sim(lists, name, W):
    if (name, W) not in _sims:
        _sims[(name, W)] = QM.simulate(lists[name], W, K)
    return _sims[(name, W)]


def test_lists(res, lists):
    n = len(lists["cases"])
    assert n == len(BC.jobs()[0]) == 1295
    order = QM.front_loaded_order(res["reason"])
    heavy = int((res["reason"] == 4).sum())
    assert len(order) == 8 * heavy and QM.range_start(len(order), 1) == heavy
    assert (res["reason"][order[:heavy]] == 4).all() and (res["reason"][order[heavy:]] != 4).all()
    assert set(order.tolist()) == set(range(n))                      # every job of the case list is in it
    assert [QM.range_start(n, r) for r in range(9)] == [n * r // 8 for r in range(9)] and QM.range_start(n, 8) == n


@pytest.mark.parametrize("name", ["cases", "front-loaded"])
@pytest.mark.parametrize("W", WAVES_PER_RANGE)
def test_every_job_is_handed_out_once(lists, name, W):
    p = lists[name]
    n = len(p)
    s = _sim(lists, name, W)
    assert (s["handed"] == 1).all() and (s["runner"] >= 0).all()
    ln = np.array([QM.range_start(n, r + 1) - QM.range_start(n, r) for r in range(8)])
    assert (s["counters"] >= ln).all() and (s["counters"] <= ln + 8 * W * K).all(), s["counters"]
    # a wavefront asks a range again only while its draws come back whole: one short draw per range at most
    assert int(np.minimum(s["counters"], ln).sum()) == n
    # the rounds add up to what the keypoints need: a round runs one iteration of each live slot (K = 2: two, or one beside an idle slot)
    assert s["rounds"].sum() * 2 - s["idle_rounds"] == p.sum()


@pytest.mark.parametrize("name", ["cases", "front-loaded"])
@pytest.mark.parametrize("W", WAVES_PER_RANGE)
def test_idle_slots_only_after_the_ranges_are_exhausted(lists, name, W):
    s = _sim(lists, name, W)
    assert s["idle_before_end"] == 0, (s["idle_before_end"], s["idle_rounds"])


@pytest.mark.parametrize("name", ["cases", "front-loaded"])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_no_more_rounds_than_the_static_chunks(modsx, lists, name, W):
    p = lists[name]
    g = modsx.baumberg_geometry(len(p))
    assert g["kernel"] == 0 and g["chunk"] == 2
    static = QM.static_rounds(BC.schedule(p, g["chunk"], K))
    s = _sim(lists, name, W)
    floor = (int(p.sum()) + K - 1) // K                                # every round with both slots live
    print(name, W, "rounds: queue", int(s["rounds"].sum()), "static", static, "floor", floor)
    assert floor <= s["rounds"].sum() <= static


@pytest.mark.parametrize("name", ["cases", "front-loaded"])
def test_more_slots_than_jobs_is_the_static_pairing(lists, name):
    """400 wavefronts per range: 6 400 slots for at most 2 744 jobs.  Every job is drawn in the first round, nothing is refilled."""
    p = lists[name]
    s = _sim(lists, name, 400)
    assert 8 * 400 * K > len(p)
    per_wave = np.bincount(s["runner"], minlength=8 * 400)
    assert per_wave.max() <= K
    longest = np.zeros(8 * 400, np.int64)
    np.maximum.at(longest, s["runner"], p)
    assert np.array_equal(s["rounds"], longest)                          # a wavefront runs as long as its longest job
    assert s["rounds"].max() == p.max() and (int(p.sum()) + K - 1) // K <= s["rounds"].sum() <= p.sum()
    assert not QM.stolen(len(p), s["runner"])[s["draws"].sum(1)[s["runner"]] == 1].any()   # whoever drew once drew from its own range


def test_stealing_happens(lists):
    p = lists["cases"]
    hit = {W: int(QM.stolen(len(p), _sim(lists, "cases", W)["runner"]).sum()) for W in (1, 2, 3, 8)}
    print(hit)
    assert all(v >= 10 for v in hit.values()), hit


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_front_loaded_list_is_drained_by_the_other_ranges(lists, W):
    p = lists["front-loaded"]
    n = len(p)
    s = _sim(lists, "front-loaded", W)
    first = QM.range_start(n, 1)
    took = QM.stolen(n, s["runner"])[:first]
    thieves = set((s["runner"][:first][took] % 8).tolist())
    print(W, "jobs of range 0 run by other ranges:", int(took.sum()), "of", first, "home ranges of the runners:", sorted(thieves))
    assert took.sum() >= first // 2 and thieves == set(range(1, 8))
