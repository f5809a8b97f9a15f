// kernels_fginn_l1.hip -- the exact search of MatchFlannFGINN (matching/matching.cpp:357-461, vector_matcher = linear) under
// vector_dist = L1 on rows that hold the integers 0..255 at 128 columns (the SIFT family), as bytes, for gfx950.
//
// Contract (include/modsx.h holds the caller's side): the one of kernels_fginn32.hip with FLANN's L1<float> chain,
// r = r + (((|e0| + |e1|) + |e2|) + |e3|) in f32.  On this domain every |e| is an integer <= 255, every group sum <= 1020 and every
// running sum <= 32640: all exact in f32, whatever the order.  The integer sum of absolute differences, converted to f32, IS the
// chain's result, so the distance here is 32 v_sad_u8 (|a - b| over four bytes plus an accumulator, __builtin_amdgcn_sad_u8) and one
// v_cvt_f32_u32.  L1 is no dot product: the matrix cores of kernels_match.hip cannot be used.
//
// Everything behind the distance is that of kernels_fginn32.hip, by the same code (search_dev.hpp): key = f32_key((float)sum, idx),
// the K = 4 smallest keys per query and split (k_l1_topk fills a Top4), k_f32_merge itself, the host walk, the F32Open / F32Closed
// records and the resolve sweep (k_l1_resolve hands (float)sum to the F32Resolve that k_f32_resolve hands its distance to).  The geometry and the workspace are those of the
// f32 search at a row of 32 dwords: fginn_l1_geometry = fginn32_geometry at DK = 32, 128 trains (16 KiB) per LDS tile.
//
// Layout.  k_l1_pack turns dense [n][128] u8 rows of any byte alignment into 16-byte-aligned rows of 8 uint4, the train side padded
// with zero rows to whole tiles (never visited).  l1_sweep: one query per lane with its row in 32 VGPRs, 256-thread workgroups, the
// next tile fetched into registers while this one is swept, every lane reads the same train words (broadcast ds_read_b128).
//
// Compiler figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; regenerated with the shared pieces in
// place: unchanged, and so is the ISA of all three kernels):
//   kernel                VGPRs  SGPRs  LDS [B]  scratch  occupancy [waves/SIMD]
//   k_l1_topk                86     25    16384        0      5
//   k_l1_resolve             88     34    16384        0      5
//   k_l1_pack                 8     12        0        0      8
// The sweep loop of k_l1_topk is unrolled over two trains.  Per (query, train) it issues 8 ds_read_b128 and 36.5 vector instructions
// when no key is inserted (32 v_sad_u8, v_cvt_f32_u32, a v_mov_b32 for the index, the 64-bit compare with the fourth key, half a
// loop compare); the insertion (7 v_cmp_*_u64, 14 v_cndmask_b32) sits behind a wave-uniform branch (s_cbranch_execz) and brings a
// pair to 57.5 where any lane takes it.  That is one ds_read_b128 per 4.6 vector instructions against one per 12 in k_f32_topk<128>
// (measured times 9.21).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "engine.hpp"
#include "search_dev.hpp"

namespace mx {

constexpr int L1_T = 128;      // trains per tile
constexpr int L1_W = 32;       // dwords per row
constexpr int L1_TILE4 = L1_T * L1_W / 4, L1_NLOAD = L1_TILE4 / 256;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

Fginn32Geo fginn_l1_geometry(int n1, int n2, int splits) {
  return fginn32_geometry_rows(n1, n2, 128, L1_W, L1_T, splits);      // rows of DK = 32 dwords; the split rule is shared
}

// dst: rowsPad rows of 8 uint4; rows >= n are zero
__global__ __launch_bounds__(256) void k_l1_pack(const uint8_t *__restrict__ src, int n, int rowsPad, uint4 *__restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rowsPad * 8) return;
  const int row = (int)(i / 8), k = 16 * (int)(i % 8);
  unsigned w[4] = {0u, 0u, 0u, 0u};
  if (row < n) {
    const uint8_t *p = src + (size_t)row * 128 + k;
#pragma unroll
    for (int e = 0; e < 4; e++)
      w[e] = (unsigned)p[4 * e] | ((unsigned)p[4 * e + 1] << 8) | ((unsigned)p[4 * e + 2] << 16) | ((unsigned)p[4 * e + 3] << 24);
  }
  dst[i] = make_uint4(w[0], w[1], w[2], w[3]);
}

// Sweeps the tiles [tBeg, tEnd) of `trains` for this lane's packed query row (null: a lane without a query; it still takes part in
// the staging) and hands consume((float)sum of absolute differences, train index) every train below n2.
template <class F>
__device__ __forceinline__ void l1_sweep(const u32x4 *__restrict__ qrow, const u32x4 *__restrict__ trains, int n2, int tBeg, int tEnd,
                                         u32x4 *__restrict__ tile, F &&consume) {
  const int tid = threadIdx.x;
  unsigned a[L1_W];
#pragma unroll
  for (int k = 0; k < L1_W / 4; k++) {
    const u32x4 v = qrow ? qrow[k] : u32x4{0u, 0u, 0u, 0u};
    a[4 * k] = v.x; a[4 * k + 1] = v.y; a[4 * k + 2] = v.z; a[4 * k + 3] = v.w;
  }
  u32x4 nxt[L1_NLOAD];
#pragma unroll
  for (int i = 0; i < L1_NLOAD; i++) nxt[i] = trains[(size_t)tBeg * L1_TILE4 + i * 256 + tid];
  for (int t = tBeg; t < tEnd; t++) {
    __syncthreads();                                   // the previous tile is no longer read
#pragma unroll
    for (int i = 0; i < L1_NLOAD; i++) tile[i * 256 + tid] = nxt[i];
    __syncthreads();
    if (t + 1 < tEnd) {
#pragma unroll
      for (int i = 0; i < L1_NLOAD; i++) nxt[i] = trains[(size_t)(t + 1) * L1_TILE4 + i * 256 + tid];
    }
    const int base = t * L1_T, jn = min(L1_T, n2 - base);
#pragma unroll 2
    for (int j = 0; j < jn; j++) {
      unsigned sum = 0;
#pragma unroll
      for (int k = 0; k < L1_W / 4; k++) {
        const u32x4 v = tile[j * (L1_W / 4) + k];
        sum = __builtin_amdgcn_sad_u8(a[4 * k], v.x, sum);
        sum = __builtin_amdgcn_sad_u8(a[4 * k + 1], v.y, sum);
        sum = __builtin_amdgcn_sad_u8(a[4 * k + 2], v.z, sum);
        sum = __builtin_amdgcn_sad_u8(a[4 * k + 3], v.w, sum);
      }
      consume((float)sum, base + j);
    }
  }
}

// keys: [S][n1][4].  Split blockIdx.y sweeps the tiles [y * tilesPerSplit, ...).
__global__ __launch_bounds__(256) void k_l1_topk(const uint4 *__restrict__ queries, int n1, const uint4 *__restrict__ trains, int n2, int ntiles,
                                                 int tilesPerSplit, unsigned long long *__restrict__ keys) {
  __shared__ __attribute__((aligned(16))) u32x4 tile[L1_TILE4];
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int t0 = blockIdx.y * tilesPerSplit, t1 = min(ntiles, t0 + tilesPerSplit);
  Top4 top;
  l1_sweep(q < n1 ? reinterpret_cast<const u32x4 *>(queries) + (size_t)q * (L1_W / 4) : nullptr, reinterpret_cast<const u32x4 *>(trains), n2,
           t0, t1, tile, [&](float d, int idx) { top.put_below(f32_key(d, idx)); });
  if (q < n1) top.store(keys + ((size_t)blockIdx.y * n1 + q) * 4);
}

// k_f32_resolve on byte rows: open[u] an undecided query; closed[u] (kterm = all ones, cnt = 0 on entry) receives over all splits the
// smallest key of a terminal train and the count of non-terminal trains among the trains with key > klast.  pos: [n2][2] f64.
__global__ __launch_bounds__(256) void k_l1_resolve(const uint4 *__restrict__ queries, const F32Open *__restrict__ open, int nu,
                                                    const uint4 *__restrict__ trains, int n2, int ntiles, int tilesPerSplit,
                                                    const double *__restrict__ pos, double contrDistSq, F32Closed *__restrict__ closed) {
  __shared__ __attribute__((aligned(16))) u32x4 tile[L1_TILE4];
  const int u = blockIdx.x * 256 + threadIdx.x;
  const int t0 = blockIdx.y * tilesPerSplit, t1 = min(ntiles, t0 + tilesPerSplit);
  F32Resolve r(open, u, u < nu, pos, contrDistSq);
  l1_sweep(u < nu ? reinterpret_cast<const u32x4 *>(queries) + (size_t)r.o.q * (L1_W / 4) : nullptr, reinterpret_cast<const u32x4 *>(trains), n2,
           t0, t1, tile, [&](float d, int idx) { r.step(d, idx); });
  r.commit(closed, u, u < nu);
}

// work: fginn32_workspace_bytes(g, n1), 256-byte aligned.  n1 >= 1, n2 >= 1.  ev (optional): three events -- before the packing,
// between the packing and the search (k_l1_topk + k_f32_merge), behind the search
void launch_fginn_l1_topk(hipStream_t s, const Fginn32Geo &g, const uint8_t *d1, int n1, const uint8_t *d2, int n2, void *work,
                          void *flagAndTop4, hipEvent_t *ev) {
  const Fginn32Work w = fginn32_work(g, n1, work);
  const int qRows = g.gx * 256, tRows = g.ntiles * g.tile;
  hipMemsetAsync(flagAndTop4, 0, 16, s);
  if (ev) hipEventRecord(ev[0], s);
  hipLaunchKernelGGL(k_l1_pack, dim3((unsigned)(((size_t)qRows * 8 + 255) / 256)), dim3(256), 0, s, d1, n1, qRows, (uint4 *)w.queries);
  hipLaunchKernelGGL(k_l1_pack, dim3((unsigned)(((size_t)tRows * 8 + 255) / 256)), dim3(256), 0, s, d2, n2, tRows, (uint4 *)w.trains);
  if (ev) hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(k_l1_topk, dim3(g.gx, g.S), dim3(256), 0, s, (const uint4 *)w.queries, n1, (const uint4 *)w.trains, n2, g.ntiles,
                     g.tilesPerSplit, w.keys);
  launch_fginn32_merge(s, g, w.keys, n1, (unsigned long long *)((char *)flagAndTop4 + 16));
  if (ev) hipEventRecord(ev[2], s);
}

// the packed rows of the last launch_fginn_l1_topk on this workspace are reused; the caller has set w.open[0 .. nu) and
// w.closed[0 .. nu) = {all ones, 0}
void launch_fginn_l1_resolve(hipStream_t s, const Fginn32Geo &g, int n1, int nu, int n2, const double *pos, double contrDistSq, void *work) {
  const Fginn32Work w = fginn32_work(g, n1, work);
  hipLaunchKernelGGL(k_l1_resolve, dim3((nu + 255) / 256, g.S), dim3(256), 0, s, (const uint4 *)w.queries, w.open, nu, (const uint4 *)w.trains,
                     n2, g.ntiles, g.tilesPerSplit, pos, contrDistSq, w.closed);
}

}  // namespace mx
