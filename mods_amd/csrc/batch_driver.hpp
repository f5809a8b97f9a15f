// batch_driver.hpp -- the host thread logic of the multi-context batch calls (capi.hip), in one copy.  Plain C++17 and POSIX: nothing
// of HIP or of the engine is included, so tests/batch_driver_main.cpp exercises it with the host compiler alone (also under
// -fsanitize=thread).  Two layers: run_groups hands groups of items to one worker per context; run_batch puts a task queue with
// helper threads on top of it.
#pragma once
#include <time.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace mx {

// n items over n_ctx >= 1 contexts: consecutive groups of `group` items come off a shared counter (the group shrinks so that all
// contexts get work when the batch is small), `nw` workers take them
struct BatchShape { int group, nw; };
inline BatchShape batch_shape(int n_ctx, int n, int group_cap) {
  const int group = std::max(1, std::min((n + n_ctx - 1) / n_ctx, group_cap));
  return {group, std::min(n_ctx, (n + group - 1) / group)};
}

struct BatchError {
  int rc = 0;           // the first non-zero code a body returned, 0: none
  std::string text;     // err_text() of the thread that returned it
};

// body(w, first, count) -> 0 or an error code, for worker w and the items first .. first + count - 1.  Worker 0 runs on the calling
// thread (its HIP device and thread-local error text are the caller's), the others on threads of their own.  After a failure no
// worker takes another group; the first failure is kept with the text err_text() gives on the failing thread.  after(w) runs on
// every worker's thread behind its last group.  Returns when all threads are joined; n == 0 runs nothing and starts no thread.
template <class Body, class ErrText, class After>
BatchError run_groups(int n_ctx, int n, int group_cap, Body &&body, ErrText &&err_text, After &&after) {
  const BatchShape s = batch_shape(n_ctx, n, group_cap);
  std::atomic<int> next(0), failed(0);
  std::mutex mu;
  BatchError err;
  auto worker = [&](int w) {
    while (!failed.load()) {      // another group failed: the batch is lost, stop feeding the stream
      const int first = next.fetch_add(s.group);
      if (first >= n) break;
      const int rc = body(w, first, std::min(s.group, n - first));
      if (rc) {
        std::lock_guard<std::mutex> lk(mu);
        if (!failed.exchange(rc)) { err.rc = rc; err.text = err_text(); }
      }
    }
    after(w);
  };
  std::vector<std::thread> th;
  for (int w = 1; w < s.nw; w++) th.emplace_back(worker, w);
  if (s.nw > 0) worker(0);
  for (auto &t : th) t.join();
  return err;
}

template <class Task>
class TaskQueue {
  std::mutex m;
  std::condition_variable cv;
  std::deque<Task> q;
  bool closed = false;

 public:
  // moves the tasks in; one task wakes one waiting thread, several wake all
  void push(std::vector<Task> &tasks) {
    if (tasks.empty()) return;
    { std::lock_guard<std::mutex> lk(m); for (Task &t : tasks) q.push_back(std::move(t)); }
    if (tasks.size() == 1) cv.notify_one(); else cv.notify_all();
  }
  // wait: block until a task is there or the queue is closed.  false: nothing queued (and, with wait, nothing will come)
  bool take(Task &t, bool wait) {
    std::unique_lock<std::mutex> lk(m);
    if (wait) cv.wait(lk, [&] { return closed || !q.empty(); });
    if (q.empty()) return false;
    t = std::move(q.front());
    q.pop_front();
    return true;
  }
  void close() {
    { std::lock_guard<std::mutex> lk(m); closed = true; }
    cv.notify_all();
  }
};

// adds the CPU time (not wall) of the calling thread between construction and destruction to acc
struct ThreadCpu {
  std::atomic<long> &acc;
  long t0;
  static long now_us() { timespec t; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t); return t.tv_sec * 1000000L + t.tv_nsec / 1000; }
  explicit ThreadCpu(std::atomic<long> &a) : acc(a), t0(now_us()) {}
  ~ThreadCpu() { acc += now_us() - t0; }
};

// what the last run_batch on this object did (measurement hooks)
struct BatchStats {
  std::atomic<long> taskUs{0};                        // add(): summed wall time of the tasks
  std::atomic<int> tasks{0}, workers{0};              // tasks consumed; nw of the run
  std::atomic<long> cpuWorkerUs{0}, cpuHelperUs{0};   // CPU time by kind of thread: producing and draining workers, helpers
  std::mutex eachMu;
  std::vector<int> eachUs;                            // add(): every task's time, in completion order
  void reset(int nw) {
    taskUs = 0; tasks = 0; workers = nw; cpuWorkerUs = 0; cpuHelperUs = 0;
    std::lock_guard<std::mutex> lk(eachMu);
    eachUs.clear();
  }
  void add(long us) {      // the consumer's report of one task
    taskUs += us;
    tasks++;
    std::lock_guard<std::mutex> lk(eachMu);
    eachUs.push_back((int)us);
  }
};

// run_groups with a queue behind it: produce(w, first, count, out) -> rc appends up to `count` tasks for its group to `out`, and
// consume(task) runs on helper threads while the workers go on to their next group.  A worker that is out of groups helps with what
// is still queued (the tail of a batch is the consumption of its last tasks, with the producers' device already idle).  The tasks
// of a group whose produce failed are dropped, not consumed.  helper_cap > 0 bounds the helper threads, otherwise there is one per
// worker.  Returns when the queue is empty and every thread is joined; stats describes this run from its start.
template <class Task, class Produce, class Consume, class ErrText>
BatchError run_batch(int n_ctx, int n, int group_cap, int helper_cap, BatchStats &stats, Produce &&produce, Consume &&consume,
                     ErrText &&err_text) {
  const int nw = batch_shape(n_ctx, n, group_cap).nw;
  stats.reset(nw);
  TaskQueue<Task> queue;
  auto drain = [&](bool wait, std::atomic<long> &cpu) {
    ThreadCpu tc(cpu);
    for (;;) {
      Task t;      // released before the thread waits for the next one
      if (!queue.take(t, wait)) return;
      consume(t);
    }
  };
  std::vector<std::thread> helpers;
  for (int h = 0; h < (helper_cap > 0 ? std::min(helper_cap, nw) : nw); h++) helpers.emplace_back(drain, true, std::ref(stats.cpuHelperUs));
  const BatchError err = run_groups(
      n_ctx, n, group_cap,
      [&](int w, int first, int count) {
        ThreadCpu tc(stats.cpuWorkerUs);
        std::vector<Task> out;
        const int rc = produce(w, first, count, out);
        if (!rc) queue.push(out);
        return rc;
      },
      err_text, [&](int) { drain(false, stats.cpuWorkerUs); });
  queue.close();
  for (auto &t : helpers) t.join();
  return err;
}

}  // namespace mx
