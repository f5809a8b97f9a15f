"""A numpy restatement of the refill rule of the queue-fed Baumberg kernel (mods_amd/csrc/kernels_affine.hip, k_baumberg_stream with
QUEUE = true; variant 3 of baumberg_geometry), and the front-loaded job list its tests share.  No GPU in here.

The rule: the job list is cut into R = 8 contiguous ranges, range r = jobs n r // 8 .. n (r + 1) // 8, each with a counter.  A
wavefront has K slots and starts on range (its index) % 8.  At the head of every round it makes ONE draw for all its idle slots: it
adds their number to the counter of its current range and gets the old value back; the idle slots take old + rank, in slot order,
while that is inside the range.  A draw that comes back short marks the range exhausted for this wavefront, which goes on to the
next range it has not seen empty and draws for the slots still idle; with all eight marked it draws no more.  A round with no
live slot ends the wavefront.

Wavefronts run in lock step here, draws in wavefront order within a round: one of the interleavings the hardware may produce (no
wavefront waits for another, so every interleaving is allowed; which one happens changes who runs a keypoint and nothing else).
"""
import numpy as np

R = 8


def range_start(n, r):
    return n * r // R


def simulate(passes, waves_per_range, K=2):
    """passes[k] = rounds keypoint k occupies a slot (>= 1).  -> dict:
      handed [n]        times job k was handed to a slot
      runner [n]        wavefront that ran job k (-1: nobody)
      rounds [waves]    rounds every wavefront ran (with at least one live slot)
      idle_rounds       rounds with a live and an idle slot, over all wavefronts
      idle_before_end   those of them at whose head some counter was still below the length of its range
      counters [R]      the counters at the end
      draws [waves, R]  draws every wavefront made on every range"""
    n = len(passes)
    waves = R * waves_per_range
    lo = [range_start(n, r) for r in range(R)]
    ln = [range_start(n, r + 1) - range_start(n, r) for r in range(R)]
    counters = [0] * R
    handed, runner = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    rounds, draws = np.zeros(waves, np.int64), np.zeros((waves, R), np.int64)
    job = [[-1] * K for _ in range(waves)]
    left = [[0] * K for _ in range(waves)]
    cur = [w % R for w in range(waves)]
    empty = [0] * waves
    running = list(range(waves))
    idle_rounds = idle_before_end = 0
    while running:
        still = []
        for w in running:
            idle = [q for q in range(K) if job[w][q] < 0]
            need, done = len(idle), 0
            while need > 0 and empty[w] != (1 << R) - 1:
                r = cur[w]
                got = counters[r]
                counters[r] += need
                draws[w, r] += 1
                avail = 0 if got >= ln[r] else min(need, ln[r] - got)
                for i in range(avail):
                    k = lo[r] + got + i
                    q = idle[done + i]
                    job[w][q], left[w][q] = k, int(passes[k])
                    handed[k] += 1
                    runner[k] = w
                done += avail
                need -= avail
                if need > 0:
                    empty[w] |= 1 << r
                    t = 1
                    while t < R and (empty[w] >> cur[w]) & 1:
                        cur[w] = (cur[w] + 1) % R
                        t += 1
            live = [q for q in range(K) if job[w][q] >= 0]
            if not live:
                continue
            rounds[w] += 1
            if len(live) < K:
                idle_rounds += 1
                idle_before_end += any(counters[r] < ln[r] for r in range(R))
            for q in live:
                left[w][q] -= 1
                if left[w][q] == 0:
                    job[w][q] = -1
            still.append(w)
        running = still
    return dict(handed=handed, runner=runner, rounds=rounds, idle_rounds=idle_rounds, idle_before_end=idle_before_end,
                counters=np.array(counters, np.int64), draws=draws)


def stolen(n, runner):
    """jobs that a wavefront of another range ran: bool [n]"""
    home = np.zeros(n, np.int64)
    for r in range(R):
        home[range_start(n, r):range_start(n, r + 1)] = r
    return (runner >= 0) & (runner % R != home)


def static_rounds(schedule_waves):
    """rounds of tests/baumberg_cases.schedule(): every pass of every wavefront"""
    return sum(len(w) for w in schedule_waves)


def front_loaded_order(reason):
    """indices into the job list for a list 8 x (iteration-limit jobs) long: every iteration-limit job (reason 4: 16 rounds each)
    first, so that they fill exactly the first range, then the other jobs in their own order, repeated to the length"""
    reason = np.asarray(reason)
    heavy, light = np.nonzero(reason == 4)[0], np.nonzero(reason != 4)[0]
    assert len(heavy) > 0 and len(light) > 0
    return np.concatenate([heavy, np.resize(light, (R - 1) * len(heavy))])
