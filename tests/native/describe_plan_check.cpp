// Stand-alone run of the description stage's planner (mods_amd/csrc/describe_plan.cpp) for the sanitizers: host code only, its own
// main, never loaded into Python.  It plans every odd window size of 19..137 and the large ones, the refused size, the direct
// branch, fast extraction, and a multi-chunk list over two images at the smallest arena, fills the staged blob of every chunk into a
// buffer of exactly the layout's size, and checks the walk against the chunk rule.  Build and run (from the repository root):
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -x hip -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I mods_amd/csrc -I include tests/native/describe_plan_check.cpp \
//         mods_amd/csrc/describe_plan.cpp mods_amd/csrc/tables.cpp -o describe_plan_check && ./describe_plan_check
// The three engine symbols the planner refers to are defined here: the error text and a serial parallel-for.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "describe_plan.hpp"

static std::string g_err;
namespace mx {
void set_error(const std::string &s) { g_err = s; }
void host_parallel_for(int n, const std::function<void(int)> &fn, bool) { for (int i = 0; i < n; i++) fn(i); }
}  // namespace mx

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static modsx_region region(double x, double y, double s) {
  modsx_region r;
  memset(&r, 0, sizeof r);
  r.det_kp.x = x; r.det_kp.y = y; r.det_kp.s = s;
  r.det_kp.a11 = 1.25; r.det_kp.a12 = -0.5; r.det_kp.a21 = 0.25; r.det_kp.a22 = 0.75;
  return r;
}

// plans the whole batch chunk by chunk as describe_batch does; -> chunks planned, or -1 for a refusal.  cnt: the summed counters
static int plan_all(const std::vector<modsx_region> *regs, int n, double mrSize, int fast, size_t arena, long *cnt) {
  mx::HostMark hm;
  mx::DescBatch b;
  b.regs = regs; b.n = n; b.mrSize = mrSize; b.fast = fast;
  mx::DescCursor cur = mx::describe_windows(b);
  for (int q = 0; q < mx::DC_N; q++) cnt[q] = 0;
  int chunks = 0;
  for (; cur.img < n; chunks++) {
    mx::DescChunkPlan cp;
    const int rc = mx::describe_plan_chunk(b, cur, arena, cp, hm);
    for (int q = 0; q < mx::DC_N; q++) cnt[q] += cp.cnt[q];
    if (rc) return -1;
    // the chunk rule: within the arena unless the chunk is one window; every job's offsets inside the arenas
    CHECK(cp.windowFloats <= arena || cp.cnt[mx::DC_JOBS] - cp.cnt[mx::DC_DIRECT_JOBS] == 1);
    CHECK(!cp.jobs.empty() && cp.pfxSample.size() == cp.jobs.size() + 1);
    for (const mx::DescJob &j : cp.jobs) {
      if (!j.P) continue;
      CHECK(j.rowOfs + (size_t)j.P * j.NC <= cp.arenaB && j.gridOfs + (size_t)j.NC * j.NC <= cp.arenaC);
      CHECK(j.rows0 ? j.scratchOfs + j.P <= cp.rowStarts : j.scratchOfs + (size_t)j.P * j.P <= cp.arenaA);
      CHECK((size_t)j.tapOfs + j.ksize <= cp.taps.size() && (size_t)j.needOfs + j.NC + 164 <= cp.needTab.size() &&
            (size_t)j.coordOfs + 41 <= cp.coordTab.size());
    }
    const mx::DescBlobLayout L(cp);
    std::vector<char> blob(L.blobB);      // exactly the staged size: a write past it is the sanitizer's to find
    mx::describe_fill_blob(cp, L, blob.data());
    cur = cp.next;
  }
  return chunks;
}

int main() {
  long cnt[mx::DC_N];
  std::vector<int> sizes;
  for (int P = 19; P <= 137; P += 2) sizes.push_back(P);
  for (int P : {471, 473, 983, 985, 1023, 1025, 2083, 2329}) sizes.push_back(P);
  for (int P : sizes) {   // s = (P - 3) / 2 at mrSize = 1 gives the window P
    std::vector<modsx_region> v[1];
    for (int k = 0; k < 3; k++) v[0].push_back(region(10.5 + 100 * k, 20.25 + 70 * k, (P - 3) / 2.0));
    CHECK(mx::describe_window(v[0][0].det_kp.s, 1.0, 0) == P);
    CHECK(plan_all(v, 1, 1.0, 0, (size_t)192 << 18, cnt) == 1 && cnt[mx::DC_JOBS] == 3 && cnt[mx::DC_DIRECT_JOBS] == 0);
    CHECK(plan_all(v, 1, 1.0, 1, (size_t)192 << 18, cnt) == 1 && cnt[mx::DC_DIRECT_JOBS] == 3);
  }
  {   // the window of 513 taps: refused, counted as a chunk without jobs
    std::vector<modsx_region> v[1];
    v[0].push_back(region(50, 50, (2331 - 3) / 2.0));
    CHECK(plan_all(v, 1, 1.0, 0, (size_t)192 << 18, cnt) == -1 && cnt[mx::DC_CHUNKS] == 1 && cnt[mx::DC_JOBS] == 0);
    CHECK(g_err.find("descriptor window too large") != std::string::npos);
  }
  {   // no regions at all, and the direct branch
    std::vector<modsx_region> v[2];
    CHECK(plan_all(v, 2, 1.0, 0, (size_t)16 << 18, cnt) == 0 && cnt[mx::DC_CHUNKS] == 0);
    v[1].push_back(region(5, 5, 7.0));
    CHECK(plan_all(v, 2, 1.0, 0, (size_t)16 << 18, cnt) == 1 && cnt[mx::DC_DIRECT_JOBS] == 1 && cnt[mx::DC_CHUNKS_LATER_IMAGE] == 1);
  }
  {   // two images at the smallest arena: 60 windows of 315, one of 2083 (larger than the arena), 20 direct, 60 of 315 | 50 of 315
    std::vector<modsx_region> v[3];
    const int runs[4][2] = {{315, 60}, {2083, 1}, {0, 20}, {315, 60}};
    for (const auto &r : runs)
      for (int k = 0; k < r[1]; k++) v[0].push_back(region(20.25 + (v[0].size() * 53) % 280, 15.5 + (v[0].size() * 31) % 210, r[0] ? (r[0] - 3) / 2.0 : 7.0));
    for (int k = 0; k < 50; k++) v[2].push_back(region(3.5 + 6 * k, 230.0 - 4 * k, 156.0));
    const int chunks = plan_all(v, 3, 1.0, 0, (size_t)16 << 18, cnt);
    printf("multi-chunk list: %d chunks, %ld mid-image, %ld at a later image, %ld jobs\n", chunks, cnt[mx::DC_CHUNKS_MID_IMAGE],
           cnt[mx::DC_CHUNKS_LATER_IMAGE], cnt[mx::DC_JOBS]);
    // cuts at 42, 60, 81, 123 of image 0; 18 + 24 windows of 315 fill the fifth chunk, the sixth begins inside image 2
    CHECK(chunks == 6 && cnt[mx::DC_CHUNKS] == 6 && cnt[mx::DC_CHUNKS_MID_IMAGE] == 5 && cnt[mx::DC_CHUNKS_LATER_IMAGE] == 1);
    CHECK(cnt[mx::DC_JOBS] == 191 && cnt[mx::DC_DIRECT_JOBS] == 20);
  }
  printf("describe_plan_check: %s (%d sizes)\n", fails ? "FAILED" : "ok", (int)sizes.size());
  return fails ? 1 : 0;
}
