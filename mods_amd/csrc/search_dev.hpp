// search_dev.hpp -- the device pieces the exact searches have in common, in one copy each: kernels_fginn32.hip (single and grouped),
// kernels_fginn_l1.hip and kernels_hamming.hip (single and grouped) include it.  Everything here is __forceinline__ code over
// scalars: the kernels compile to the instructions they had when each of them wrote these bodies out.  The sweeps
// (f32_sweep, l1_sweep, ham_sweep) are different loops on different row types and stay with their files.
#pragma once
#include <hip/hip_runtime.h>
#include "engine.hpp"

namespace mx {

// the key of a (distance, train index): distances are >= +0 and never NaN, so the pattern orders like the value; all ones = no train
constexpr unsigned long long F32_NONE = ~0ull;
__device__ __forceinline__ unsigned long long f32_key(float d, int idx) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)idx;
}

// The K = 4 smallest keys met, in order.  Keys are unique per train, so the branch-free insertion needs no tie rule.
struct Top4 {
  unsigned long long k0 = F32_NONE, k1 = F32_NONE, k2 = F32_NONE, k3 = F32_NONE;
  __device__ __forceinline__ void put(unsigned long long key) {
    k3 = min(k3, max(k2, key));
    k2 = min(k2, max(k1, key));
    k1 = min(k1, max(k0, key));
    k0 = min(k0, key);
  }
  // the sweeps' form: most keys fail the one compare with the fourth
  __device__ __forceinline__ void put_below(unsigned long long key) {
    if (key < k3) put(key);
  }
  __device__ __forceinline__ void store(unsigned long long *o) const { o[0] = k0; o[1] = k1; o[2] = k2; o[3] = k3; }
};

// out[0..4) = the four smallest of query q's keys over the splits [s0, s1) of keys [splits][n1][4] (all ones where there is none)
__device__ __forceinline__ void f32_merge_splits(const unsigned long long *keys, int n1, int q, int s0, int s1, unsigned long long *out) {
  Top4 top;
  for (int s = s0; s < s1; s++) {
    const unsigned long long *p = keys + ((size_t)s * n1 + q) * 4;
#pragma unroll
    for (int e = 0; e < 4; e++) top.put(p[e]);
  }
  top.store(out);
}

// the Hamming searches' merge: *out = {first, d(first), second, d(second)} from the two smallest of query q's keys
// (distance << 32) | index over the splits [s0, s1) of part [splits][n1][2] (-1, -1 where there is none)
__device__ __forceinline__ void ham_merge_splits(const unsigned long long *part, int n1, int q, int s0, int s1, int4 *out) {
  unsigned long long k1 = ~0ull, k2 = ~0ull;
  for (int s = s0; s < s1; s++) {
    const unsigned long long *p = part + ((size_t)s * n1 + q) * 2;
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const unsigned long long k = p[e];
      k2 = min(k2, max(k1, k));
      k1 = min(k1, k);
    }
  }
  int4 r;
  r.x = k1 == ~0ull ? -1 : (int)(k1 & 0xffffffffu); r.y = k1 == ~0ull ? -1 : (int)(k1 >> 32);
  r.z = k2 == ~0ull ? -1 : (int)(k2 & 0xffffffffu); r.w = k2 == ~0ull ? -1 : (int)(k2 >> 32);
  *out = r;
}

// One lane of a resolve sweep: open[u] is an undecided query (fginn_walk.hpp); over the trains with key > klast it keeps the smallest
// key of a terminal train (d >= d_pass, or farther than contradDist from train t0 in f64) and the count of the others, and commits
// them to closed[u] (kterm = all ones, cnt = 0 on entry) with integer atomics, so the splits may arrive in any order.  A lane that
// is not live sweeps with an entry no train can pass (klast = all ones) and commits nothing.  pos: [n2][2] f64.
struct F32Resolve {
  F32Open o;
  const double *__restrict__ pos;
  double px, py, contrDistSq;
  unsigned long long kterm = F32_NONE;
  unsigned cnt = 0;
  __device__ __forceinline__ F32Resolve(const F32Open *__restrict__ open, int u, bool live, const double *__restrict__ pos_, double cd2)
      : pos(pos_), contrDistSq(cd2) {
    o.klast = F32_NONE; o.q = 0; o.t0 = 0; o.dpass = 0.f; o.pad = 0;
    if (live) o = open[u];
    px = pos[2 * (size_t)o.t0]; py = pos[2 * (size_t)o.t0 + 1];
  }
  __device__ __forceinline__ void step(float d, int idx) {
    const unsigned long long key = f32_key(d, idx);
    const double dx = px - pos[2 * (size_t)idx], dy = py - pos[2 * (size_t)idx + 1];
    const bool terminal = d >= o.dpass || dx * dx + dy * dy > contrDistSq;
    if (key > o.klast) {
      if (terminal) kterm = min(kterm, key);
      else cnt++;
    }
  }
  __device__ __forceinline__ void commit(F32Closed *__restrict__ closed, int u, bool live) const {
    if (live) {
      if (kterm != F32_NONE) atomicMin(&closed[u].kterm, kterm);
      if (cnt) atomicAdd(&closed[u].cnt, cnt);
    }
  }
};

// The grouped forms' by-value tables (F32Group, HamGroup).  group_pick: element p of a table -- compares and selects on constant
// indices, so the table stays in scalar registers.  group_problem: the problem that owns split (or resolve workgroup) y, given the
// problems' first splits; entries behind the last problem hold the total, so no workgroup selects an unused one.
static_assert(MATCH_MAXB == 4, "group_pick and group_problem are written for four problems");
template <class T>
__device__ __forceinline__ T group_pick(const T *a, int p) {
  T v = a[0];
  if (p == 1) v = a[1];
  if (p == 2) v = a[2];
  if (p == 3) v = a[3];
  return v;
}
__device__ __forceinline__ int group_problem(const int *first, int y) { return (y >= first[1]) + (y >= first[2]) + (y >= first[3]); }

}  // namespace mx
