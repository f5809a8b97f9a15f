// fginn_walk.hpp -- the host side of MatchFlannFGINN on f32 keys (matching/matching.cpp:385-457, ratio^2 < 1), in one copy: the walk
// over the four nearest keys of every query with the reference's f32 division and f64 contradiction test, the entry an open walk
// sends to the resolve sweep (k_f32_resolve and its kin), the rule that reads the sweep's answer, and the record.  The single call
// (engine_fginn32.hip) and the grouped call of the stored float classes (engine_reps_f32.hip) run these three steps around their
// own launches.  Plain C++17: only the standard library and modsx.h (for modsx_tentative) are included, so tests/fginn_walk_main.cpp
// runs the walk with the host compiler alone (also under -fsanitize=address,undefined).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <iterator>
#include <vector>
#include "../../include/modsx.h"

namespace mx {

// an undecided query on its way to the resolve sweep (pad: its problem), and what comes back.  The kernels read the same layout
struct F32Open { unsigned long long klast; int q, t0; float dpass; int pad; };
struct F32Closed { unsigned long long kterm; unsigned cnt, pad; };

// a key is (f32 distance bits << 32) | train index; all ones = no train
constexpr unsigned long long KEY_NONE = ~0ull;
inline float key_dist(unsigned long long k) { const uint32_t b = (uint32_t)(k >> 32); float f; memcpy(&f, &b, 4); return f; }
inline int key_idx(unsigned long long k) { return (int)(uint32_t)k; }

// (double)(d0 / d) <= ratio^2 with the f32 division of matching.cpp:392: the ratio test of the walk
inline bool ratio_passes(float d0, float d, double rsq, double *ratio) {
  const double r = d0 / d;
  if (ratio) *ratio = r;
  return r <= rsq;
}

// The smallest f32 d > 0 with (double)(d0 / d) <= rsq, by bisection over the bit patterns: the quotient does not grow with the
// divisor (rounding is monotone), d0 / inf = 0 passes (rsq >= 0), so the patterns that pass are an upper range of [1, 0x7f800000].
// d0 = 0 gives the smallest subnormal: 0 / d = 0 passes for every d > 0, 0 / 0 is NaN and passes nothing.  d0 >= 0 and finite.
inline float fginn32_dpass(float d0, double rsq) {
  uint32_t lo = 1, hi = 0x7f800000u;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    float d;
    memcpy(&d, &mid, 4);
    if (ratio_passes(d0, d, rsq, nullptr)) hi = mid; else lo = mid + 1;
  }
  float d;
  memcpy(&d, &lo, 4);
  return d;
}

inline modsx_tentative make_record(int q, const unsigned long long *k, unsigned long long kj, double ratio) {
  modsx_tentative t;
  t.q = q; t.t0 = key_idx(k[0]); t.tj = key_idx(kj); t.t1 = key_idx(k[1]);
  t.d1 = key_dist(k[0]); t.d2 = key_dist(kj); t.d2by2ndcl = key_dist(k[1]);
  t.ratio = sqrt(ratio);
  return t;
}

// One problem's walk.  early: the records of the open step; late: those of the close step; both in query order, no query in both.
// stage [n1]: how the query was closed (Fginn32Tap): 0 the open step, 1 the resolve sweep, 2 the sweep's count
struct FginnWalk {
  std::vector<modsx_tentative> early, late;
  std::vector<unsigned char> stage;
};

// The open step of problem `prob`: top4 [n1][4] its keys, pos2 [n2][2] f64 its trains' positions on the host.  Every query that
// ends within j <= min(3, nn - 1) is decided here; with nn - 1 > 3 the others are appended to `open`.
inline void fginn_walk_open(const unsigned long long *top4, int n1, const double *pos2, double rsq, double cd2, int nn, int prob,
                            FginnWalk &w, std::vector<F32Open> &open) {
  w.early.clear(); w.late.clear();
  w.stage.assign(n1, 0);
  const int jTop = std::min(3, nn - 1);
  for (int q = 0; q < n1; q++) {
    const unsigned long long *k = top4 + (size_t)q * 4;
    const float d0 = key_dist(k[0]);
    bool ended = k[0] == KEY_NONE;
    for (int j = 1; j <= jTop && !ended; j++) {
      if (k[j] == KEY_NONE) { ended = true; break; }            // the trains ran out (the oracle's ir[j] < 0)
      double ratio;
      if (ratio_passes(d0, key_dist(k[j]), rsq, &ratio)) { w.early.push_back(make_record(q, k, k[j], ratio)); ended = true; break; }
      const int i0 = key_idx(k[0]), ij = key_idx(k[j]);
      const double dx = pos2[2 * (size_t)i0] - pos2[2 * (size_t)ij], dy = pos2[2 * (size_t)i0 + 1] - pos2[2 * (size_t)ij + 1];
      if (dx * dx + dy * dy > cd2) ended = true;
    }
    if (ended || nn - 1 <= 3) continue;
    F32Open o;
    o.klast = k[3]; o.q = q; o.t0 = key_idx(k[0]); o.dpass = fginn32_dpass(d0, rsq); o.pad = prob;
    open.push_back(o);
    w.stage[q] = 1;
  }
}

// The close step over every problem's open entries: closed[u] answers open[u] (kterm: the smallest key behind klast of a train that
// ends the walk, all ones: none; cnt: the trains behind klast that do not).  top4: the keys of all problems, [pad][n1][4]; walks
// [pad].  Returns how many queries the count closed.
inline int fginn_walk_close(const std::vector<F32Open> &open, const F32Closed *closed, const unsigned long long *top4, int n1, double rsq,
                            int nn, FginnWalk *walks) {
  int nByCount = 0;
  for (size_t u = 0; u < open.size(); u++) {
    const F32Open &o = open[u];
    const unsigned long long kt = closed[u].kterm;
    if (kt == KEY_NONE) continue;                               // nothing ends the walk before the trains or the nn run out
    const unsigned long long *k = top4 + ((size_t)o.pad * n1 + o.q) * 4;
    double ratio;
    if (!ratio_passes(key_dist(k[0]), key_dist(kt), rsq, &ratio)) continue;      // it ends the walk by contradiction, reached or not
    // it passes, so d >= d_pass, and every non-terminal train (d < d_pass) comes before it: its rank is 3 + cnt + 1 exactly
    if ((long)closed[u].cnt + 4 <= nn - 1) walks[o.pad].late.push_back(make_record(o.q, k, kt, ratio));
    else { walks[o.pad].stage[o.q] = 2; nByCount++; }           // the nn run out first
  }
  return nByCount;
}

// The emit step: the problem's records in query order
inline void fginn_walk_emit(const FginnWalk &w, std::vector<modsx_tentative> &out) {
  out.clear();
  out.reserve(w.early.size() + w.late.size());
  std::merge(w.early.begin(), w.early.end(), w.late.begin(), w.late.end(), std::back_inserter(out),
             [](const modsx_tentative &a, const modsx_tentative &b) { return a.q < b.q; });
}

}  // namespace mx
