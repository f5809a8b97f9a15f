// Stand-alone check of mods_amd/csrc/batch_driver.hpp (tests/test_batch_driver_cpu.py builds it with the host compiler, plain and
// under -fsanitize=thread, and runs it as a child under a time limit: a deadlock is a timeout).  Only the header and the standard
// library; the task is a pair of ints.  Every shape and failure set runs `reps` times (argv[1], default 40) in each of up to seven
// forms, with small random sleeps in the producers and consumers that vary the schedule.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include "../mods_amd/csrc/batch_driver.hpp"

#define CHECK(c)                                                                                          \
  do {                                                                                                    \
    if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed in %s\n", __FILE__, __LINE__, #c, g_case); exit(1); } \
  } while (0)

static char g_case[160] = "start";
static std::atomic<long> g_calls(0);      // every producer and consumer call of the process

struct Task { int item = -1, first = -1; };
enum Emit { EMIT_NONE, EMIT_ONE, EMIT_ALL };
static const int SHAPES[7][3] = {{1, 0, 4}, {1, 1, 4}, {3, 1, 4}, {2, 5, 4}, {2, 9, 4}, {4, 3, 1}, {3, 7, 1}};      // n_ctx, n, group_cap

static thread_local std::string t_err;      // the "last error" of a thread, as mx::last_error is
static thread_local unsigned t_rng = 0;
static void jitter(unsigned seed) {
  if (!t_rng) t_rng = seed * 2654435761u + 12345u;
  t_rng ^= t_rng << 13; t_rng ^= t_rng >> 17; t_rng ^= t_rng << 5;
  if (t_rng % 4 == 0) std::this_thread::sleep_for(std::chrono::microseconds(t_rng / 4 % 40));
  else if (t_rng % 4 == 1) std::this_thread::yield();
}

// the formulas of the issue, written out once more
static int want_group(int n_ctx, int n, int cap) { int g = (n + n_ctx - 1) / n_ctx; if (g > cap) g = cap; return g < 1 ? 1 : g; }
static int want_nw(int n_ctx, int n, int cap) { const int g = want_group(n_ctx, n, cap), groups = (n + g - 1) / g; return n_ctx < groups ? n_ctx : groups; }

struct Run {
  int n_ctx, n, cap, group, nw;
  std::set<int> fail;      // items whose group's producer fails (code 100 + item), after it has put its tasks into `out`
  Emit emit;
  std::vector<std::atomic<int>> produced, consumed;
  std::mutex mu;
  std::map<int, std::thread::id> workerThread;
  std::set<std::thread::id> consumerThreads;
  std::set<int> failedFirsts;      // the groups whose producer did return a failure
  std::atomic<int> pushed{0};
  Run(int n_ctx_, int n_, int cap_, Emit e) : n_ctx(n_ctx_), n(n_), cap(cap_), group(want_group(n_ctx_, n_, cap_)), nw(want_nw(n_ctx_, n_, cap_)),
                                              emit(e), produced(n_), consumed(n_) {}
  // the checks every body shares: the group's geometry, one thread per worker, each item once
  int body(int w, int first, int count) {
    g_calls++;
    jitter(first + 1);
    CHECK(w >= 0 && w < nw && first >= 0 && first < n && first % group == 0 && count == std::min(group, n - first));
    {
      std::lock_guard<std::mutex> lk(mu);
      auto it = workerThread.emplace(w, std::this_thread::get_id()).first;
      CHECK(it->second == std::this_thread::get_id());
    }
    int rc = 0;
    for (int i = first; i < first + count; i++) {
      CHECK(produced[i].fetch_add(1) == 0);
      if (!rc && fail.count(i)) rc = 100 + i;
    }
    t_err = (rc ? "failed at item " : "fine up to group ") + std::to_string(rc ? rc - 100 : first);
    if (rc) { std::lock_guard<std::mutex> lk(mu); failedFirsts.insert(first); }
    return rc;
  }
  int produce(int w, int first, int count, std::vector<Task> &out) {
    CHECK(out.empty());
    for (int i = first; i < first + (emit == EMIT_ALL ? count : emit == EMIT_ONE ? 1 : 0); i++) { out.emplace_back(); out.back().item = i; out.back().first = first; }
    const int rc = body(w, first, count);
    if (!rc) pushed += (int)out.size();
    return rc;
  }
  void consume(Task &t, mx::BatchStats &stats) {
    g_calls++;
    jitter(t.item + 77);
    CHECK(t.item >= 0 && t.item < n && consumed[t.item].fetch_add(1) == 0);
    stats.add(1);
    std::lock_guard<std::mutex> lk(mu);
    consumerThreads.insert(std::this_thread::get_id());
  }
  // after the call: nothing may move any more
  void settled(bool wait) {
    const long calls = g_calls.load();
    if (wait) std::this_thread::sleep_for(std::chrono::milliseconds(2));
    CHECK(g_calls.load() == calls);
    if (workerThread.count(0)) CHECK(workerThread[0] == std::this_thread::get_id());      // worker 0 may have met no group of its own
    std::set<std::thread::id> ids;
    for (auto &kv : workerThread) ids.insert(kv.second);
    CHECK((int)ids.size() <= nw && ids.size() == workerThread.size());
  }
  void check_error(const mx::BatchError &err) {
    if (failedFirsts.empty()) { CHECK(err.rc == 0 && err.text.empty()); return; }
    // one of the codes that were returned, with the text its own thread left
    CHECK(err.rc >= 100 && fail.count(err.rc - 100) && failedFirsts.count((err.rc - 100) / group * group));
    CHECK(err.text == "failed at item " + std::to_string(err.rc - 100));
  }
};

static void one_batch(int n_ctx, int n, int cap, int helper_cap, Emit emit, const std::set<int> &fail, bool wait) {
  Run r(n_ctx, n, cap, emit);
  r.fail = fail;
  mx::BatchStats stats;
  stats.add(5);      // left over from an earlier run: reset() must drop it
  const mx::BatchError err = mx::run_batch<Task>(
      n_ctx, n, cap, helper_cap, stats, [&](int w, int first, int count, std::vector<Task> &out) { return r.produce(w, first, count, out); },
      [&](Task &t) { r.consume(t, stats); }, [] { return t_err; });
  r.settled(wait);
  r.check_error(err);
  int consumed = 0;
  for (int i = 0; i < n; i++) {
    const bool groupFailed = r.failedFirsts.count(i / r.group * r.group) > 0;
    const int want = r.produced[i] && !groupFailed && (emit == EMIT_ALL || (emit == EMIT_ONE && i % r.group == 0)) ? 1 : 0;
    CHECK(r.consumed[i] == want);      // every pushed task once, none of a failed group
    if (fail.empty()) CHECK(r.produced[i] == 1);
    consumed += r.consumed[i];
  }
  CHECK(consumed == r.pushed.load());
  CHECK(stats.workers == r.nw && stats.tasks == consumed && (int)stats.eachUs.size() == consumed && stats.taskUs == consumed);
  CHECK((int)r.consumerThreads.size() <= r.nw + (helper_cap > 0 ? std::min(helper_cap, r.nw) : r.nw));
  if (!fail.empty() && n > 0) CHECK(!r.failedFirsts.empty());      // group 0 is always taken, and every set below fails it or is alone
}

static void one_loop(int n_ctx, int n, int cap, const std::set<int> &fail, bool wait) {
  Run r(n_ctx, n, cap, EMIT_NONE);
  r.fail = fail;
  std::atomic<int> afters(0);
  const std::thread::id caller = std::this_thread::get_id();
  const mx::BatchError err = mx::run_groups(
      n_ctx, n, cap, [&](int w, int first, int count) { return r.body(w, first, count); }, [] { return t_err; },
      [&](int w) {      // once per worker, on its thread, whether it met a group or not; worker 0 is the caller
        std::lock_guard<std::mutex> lk(r.mu);
        CHECK(r.workerThread.count(w) == 0 || r.workerThread[w] == std::this_thread::get_id());
        CHECK((w == 0) == (std::this_thread::get_id() == caller));
        afters++;
      });
  r.settled(wait);
  r.check_error(err);
  CHECK(afters == r.nw);
  for (int i = 0; i < n; i++) CHECK(fail.empty() ? r.produced[i] == 1 : r.produced[i] <= 1);
}

int main(int argc, char **argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 40;
  long runs = 0;
  for (const auto &s : SHAPES) {
    const int n_ctx = s[0], n = s[1], cap = s[2];
    const mx::BatchShape shape = mx::batch_shape(n_ctx, n, cap);
    snprintf(g_case, sizeof g_case, "shape (%d, %d, %d)", n_ctx, n, cap);
    CHECK(shape.group == want_group(n_ctx, n, cap) && shape.nw == want_nw(n_ctx, n, cap));
    // no failure; then the failing item first, in the middle, last; then two failures with different codes (the first and the last
    // item: with more than one worker both groups can be in flight at once)
    std::vector<std::set<int>> fails = {{}};
    if (n > 0) { fails.push_back({0}); fails.push_back({n / 2}); fails.push_back({n - 1}); fails.push_back({0, n - 1}); }
    for (size_t f = 0; f < fails.size(); f++)
      for (int rep = 0; rep < reps; rep++) {
        // a lone failure in a later group is met only if no earlier failure stopped the workers: it is alone, so it is met
        snprintf(g_case, sizeof g_case, "shape (%d, %d, %d) failure set %d rep %d", n_ctx, n, cap, (int)f, rep);
        one_loop(n_ctx, n, cap, fails[f], rep == 0);
        for (int helper_cap : {1, shape.nw})
          for (Emit emit : {EMIT_NONE, EMIT_ONE, EMIT_ALL}) {
            if (f > 0 && emit == EMIT_NONE && rep % 4) continue;      // failures matter most with tasks to drop
            one_batch(n_ctx, n, cap, helper_cap, emit, fails[f], rep == 0);
            runs++;
          }
      }
  }
  printf("batch driver ok: %ld batch runs\n", runs);
  return 0;
}
