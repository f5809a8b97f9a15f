// kernels_hamming.hip -- the exact search of MatchFLANNDistance (matching/matching.cpp:607-666, binary_matcher = linear,
// binary_dist = HAMMING) for gfx950: for every query row the two nearest train rows by (Hamming distance, train index).
//
// Contract of the search (the record rule that follows it is host code, engine_hamming.hip hamming_tentatives):
//   rows    nbytes bytes per region, 1 <= nbytes <= MODSX_HAMMING_MAX_BYTES (64); the reference stores Row[j] = floor(desc.vec[j])
//           as uchar, the library takes u8 rows (or f32 rows holding the integers 0..255, converted on the host)
//   result  per query {first, d(first), second, d(second)}: the two smallest of (distance, train index) in lexicographic order,
//           so equal distances keep the lower train index for the first and for the second neighbour (oracle_match.cpp knn_linear)
//   n2 == 1 is refused by the callers: the reference reads a second neighbour that was never written
//
// Layout.  k_hamming_pack turns dense [n][nbytes] u8 rows of any alignment into rows of WK dwords (W = ceil(nbytes / 4) rounded
// up to the kernel width WK in {1, 2, 4, 8, 16}), zero-filled, the array 16-byte aligned and the train side padded with zero
// rows to whole tiles.  Zero padding on both sides adds 0 to every distance.
// k_hamming_2nn<WK>: one query per lane, its WK dwords in VGPRs, 256-thread workgroups (blockIdx.x = 256 queries).  The trains pass
// through LDS in tiles of HAM_TILE_DWORDS = 1024 dwords (4 KiB: one uint4 per thread, the next tile is fetched into a register
// while this one is swept); every lane reads the same train words, a broadcast read without bank conflicts.  Per (query, train):
// WK v_xor_b32, WK v_bcnt_u32_b32 (the population count accumulates through its add operand), then
//     key = (distance << 21) | train index        distance <= 512 < 2^10, index < 2 000 000 < 2^21: 31 bits, unique per train
//     k2 = min(k2, max(k1, key)); k1 = min(k1, key)
// The 32-bit key orders exactly like (distance, index), so the update needs no visiting order and no tie rule of its own.
// The train axis is cut into S splits (gridDim.y) of whole tiles; every split writes its two best per query as 64-bit keys
// (distance << 32) | index (all ones = none).  k_hamming_merge takes the two smallest keys over the splits: integers only, the
// keys are distinct, so the result is a pure function of the inputs -- not of S, the tile length or any launch order.
// Geometry (tile length in trains, S, workgroups) comes from hamming_geometry(n1, n2, W, splits) alone; the cut of the train axis
// is split_rule (engine.hpp), the one rule of every exact search.
//
// Compiler figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; regenerated with the shared pieces in
// place: every figure is what it was, and so is the ISA of every kernel but the two merges):
//   kernel               VGPRs  SGPRs  LDS [B]  scratch  occupancy [waves/SIMD]
//   k_hamming_2nn<1>        18     27     4096        0      8
//   k_hamming_2nn<2>        22     27     4096        0      8
//   k_hamming_2nn<4>        32     27     4096        0      8
//   k_hamming_2nn<8>        52     27     4096        0      8
//   k_hamming_2nn<16>       44     25     4096        0      8
//   k_hamming_pack          11     24        0        0      8
//   k_hamming_merge         14     16        0        0      8
//   k_hamg_2nn<1>           18     27     4096        0      8
//   k_hamg_2nn<2>           22     27     4096        0      8
//   k_hamg_2nn<4>           32     27     4096        0      8
//   k_hamg_2nn<8>           52     27     4096        0      8
//   k_hamg_2nn<16>          44     25     4096        0      8
//   k_hamg_merge            14     19        0        0      8
// k_hamg_* are the grouped form at the end of the file: up to four problems of one stored query side in one launch, the sweep
// (ham_sweep) shared with k_hamming_2nn, the merge and its int4 decoding (ham_merge_splits) shared with k_hamming_merge, the
// table selection (group_pick / group_problem) shared with the grouped f32 search: the last three live in search_dev.hpp.  k_hamg_2nn asks for eight waves per SIMD in its launch bounds: without that the compiler
// gives the <16> instance 92 VGPRs (occupancy 5) where the same loop in k_hamming_2nn<16> takes 44.
// i.e. eight workgroups of 256 per CU (the 32-wave cap), 32 KiB of the CU's 160 KiB LDS.  Per (query, train) k_hamming_2nn<8>
// issues 2 WK + 3.75 vector instructions (WK v_xor_b32, WK v_bcnt_u32_b32, v_lshl_or_b32, v_max_u32, v_min_u32, half a v_min3_u32,
// a quarter of a v_mov_b32) and WK / 4 ds_read_b128 (measured times 9.8).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "engine.hpp"
#include "search_dev.hpp"

namespace mx {

constexpr int HAM_TILE_DWORDS = 1024;      // one uint4 per thread of a 256-thread workgroup
constexpr int HAM_IDX_BITS = 21;           // 2 000 000 trains at most
constexpr unsigned HAM_NONE = 0xffffffffu;

int hamming_kernel_width(int W) { return W <= 1 ? 1 : W <= 2 ? 2 : W <= 4 ? 4 : W <= 8 ? 8 : 16; }

// splits = 0: production (enough workgroups for every CU to hold its eight); splits > 0: that many, at most one per tile
// (split_rule, engine.hpp)
HammingGeo hamming_geometry(int n1, int n2, int W, int splits) {
  HammingGeo g;
  g.W = W;
  g.WK = hamming_kernel_width(W);
  g.tile = HAM_TILE_DWORDS / g.WK;
  g.ntiles = std::max(1, (n2 + g.tile - 1) / g.tile);
  g.gx = std::max(1, (n1 + 255) / 256);
  const SplitCut cut = split_rule(g.ntiles, g.gx, splits);
  g.tilesPerSplit = cut.tilesPerSplit;
  g.S = cut.S;
  return g;
}

size_t hamming_workspace_bytes(const HammingGeo &g, int n1) {
  const size_t q = ((size_t)g.gx * 256 * g.WK * 4 + 255) & ~(size_t)255;
  const size_t t = (size_t)g.ntiles * HAM_TILE_DWORDS * 4;
  const size_t p = (size_t)g.S * (size_t)n1 * 16;
  return q + t + p;
}

// dst: rowsPad rows of WK dwords; rows >= n and bytes >= nbytes are zero
__global__ __launch_bounds__(256) void k_hamming_pack(const uint8_t *__restrict__ src, int n, int nbytes, int WK, int rowsPad,
                                                      uint32_t *__restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rowsPad * WK) return;
  const int row = (int)(i / WK), w = (int)(i % WK);
  uint32_t v = 0;
  if (row < n) {
    const uint8_t *p = src + (size_t)row * nbytes;
#pragma unroll
    for (int b = 0; b < 4; b++)
      if (4 * w + b < nbytes) v |= (uint32_t)p[4 * w + b] << (8 * b);
  }
  dst[i] = v;
}

__device__ __forceinline__ unsigned long long ham_key64(unsigned k) {
  return k == HAM_NONE ? ~0ull : ((unsigned long long)(k >> HAM_IDX_BITS) << 32) | (k & ((1u << HAM_IDX_BITS) - 1));
}

// The sweep both search kernels share.  Query q's WK dwords go into VGPRs (zeros for q >= n1); the tiles [t0, t1) of `trains` (whole
// tiles, zero rows behind row n2 - 1, which the sweep never visits: jn = min(T, n2 - base)) pass through `tile`; k1 <= k2 leave as
// the two smallest 32-bit keys met, HAM_NONE where there is none.
template <int WK>
__device__ __forceinline__ void ham_sweep(const uint32_t *__restrict__ queries, int q, int n1, const uint4 *__restrict__ trains, int n2,
                                          int t0, int t1, uint32_t *tile, unsigned &k1, unsigned &k2) {
  constexpr int T = HAM_TILE_DWORDS / WK;
  const int tid = threadIdx.x;
  uint32_t a[WK];
#pragma unroll
  for (int w = 0; w < WK; w++) a[w] = 0;
  if (q < n1) {
    if constexpr (WK >= 4) {
      const uint4 *p = reinterpret_cast<const uint4 *>(queries + (size_t)q * WK);
#pragma unroll
      for (int w = 0; w < WK / 4; w++) { const uint4 v = p[w]; a[4 * w] = v.x; a[4 * w + 1] = v.y; a[4 * w + 2] = v.z; a[4 * w + 3] = v.w; }
    } else {
#pragma unroll
      for (int w = 0; w < WK; w++) a[w] = queries[(size_t)q * WK + w];
    }
  }
  k1 = HAM_NONE; k2 = HAM_NONE;
  uint4 nxt = trains[(size_t)t0 * 256 + tid];
  for (int t = t0; t < t1; t++) {
    __syncthreads();                                   // the previous tile is no longer read
    reinterpret_cast<uint4 *>(tile)[tid] = nxt;
    __syncthreads();
    if (t + 1 < t1) nxt = trains[(size_t)(t + 1) * 256 + tid];
    const int base = t * T, jn = min(T, n2 - base);
#pragma unroll 4
    for (int j = 0; j < jn; j++) {
      unsigned d = 0;
#pragma unroll
      for (int w = 0; w < WK; w++) d += __builtin_popcount(a[w] ^ tile[j * WK + w]);
      const unsigned key = (d << HAM_IDX_BITS) | (unsigned)(base + j);
      k2 = min(k2, max(k1, key));
      k1 = min(k1, key);
    }
  }
}

// part: [S][n1][2] keys.  Split blockIdx.y sweeps the tiles [y * tilesPerSplit, ...) of `trains` (ntiles whole tiles, zero rows
// behind row n2 - 1, which the sweep never visits).
template <int WK>
__global__ __launch_bounds__(256) void k_hamming_2nn(const uint32_t *__restrict__ queries, int n1, const uint4 *__restrict__ trains,
                                                     int n2, int ntiles, int tilesPerSplit, unsigned long long *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[HAM_TILE_DWORDS];
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int t0 = blockIdx.y * tilesPerSplit, t1 = min(ntiles, t0 + tilesPerSplit);
  unsigned k1, k2;
  ham_sweep<WK>(queries, q, n1, trains, n2, t0, t1, tile, k1, k2);
  if (q < n1) {
    unsigned long long *o = part + ((size_t)blockIdx.y * n1 + q) * 2;
    o[0] = ham_key64(k1);
    o[1] = ham_key64(k2);
  }
}

// nn2[q] = {first, d(first), second, d(second)}: the two smallest of the 2 S keys of query q (-1, -1 where there is none)
__global__ __launch_bounds__(256) void k_hamming_merge(const unsigned long long *__restrict__ part, int n1, int S, int4 *__restrict__ nn2) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n1) return;
  ham_merge_splits(part, n1, q, 0, S, nn2 + q);
}

template <int WK>
static void launch_2nn(hipStream_t s, const HammingGeo &g, const uint32_t *q, int n1, const uint4 *t, int n2, unsigned long long *part) {
  hipLaunchKernelGGL(k_hamming_2nn<WK>, dim3(g.gx, g.S), dim3(256), 0, s, q, n1, t, n2, g.ntiles, g.tilesPerSplit, part);
}

// d1 / d2: dense [n][nbytes] u8 rows in HBM (any alignment); work: hamming_workspace_bytes(g, n1), 256-byte aligned;
// nn2: n1 int4 in HBM.  n1 >= 1, n2 >= 1.  ev (optional): three events -- before the packing, between the packing and the search
// (k_hamming_2nn + k_hamming_merge), behind the search
void launch_hamming(hipStream_t s, const HammingGeo &g, const uint8_t *d1, int n1, const uint8_t *d2, int n2, int nbytes, void *work,
                    int *nn2, hipEvent_t *ev) {
  const size_t qB = ((size_t)g.gx * 256 * g.WK * 4 + 255) & ~(size_t)255, tB = (size_t)g.ntiles * HAM_TILE_DWORDS * 4;
  uint32_t *q = (uint32_t *)work, *t = (uint32_t *)((char *)work + qB);
  unsigned long long *part = (unsigned long long *)((char *)work + qB + tB);
  const int qRows = g.gx * 256, tRows = g.ntiles * g.tile;
  if (ev) hipEventRecord(ev[0], s);
  hipLaunchKernelGGL(k_hamming_pack, dim3((unsigned)(((size_t)qRows * g.WK + 255) / 256)), dim3(256), 0, s, d1, n1, nbytes, g.WK, qRows, q);
  hipLaunchKernelGGL(k_hamming_pack, dim3((unsigned)(((size_t)tRows * g.WK + 255) / 256)), dim3(256), 0, s, d2, n2, nbytes, g.WK, tRows, t);
  if (ev) hipEventRecord(ev[1], s);
  switch (g.WK) {
    case 1: launch_2nn<1>(s, g, q, n1, (const uint4 *)t, n2, part); break;
    case 2: launch_2nn<2>(s, g, q, n1, (const uint4 *)t, n2, part); break;
    case 4: launch_2nn<4>(s, g, q, n1, (const uint4 *)t, n2, part); break;
    case 8: launch_2nn<8>(s, g, q, n1, (const uint4 *)t, n2, part); break;
    default: launch_2nn<16>(s, g, q, n1, (const uint4 *)t, n2, part); break;
  }
  hipLaunchKernelGGL(k_hamming_merge, dim3(g.gx), dim3(256), 0, s, part, n1, g.S, (int4 *)nn2);
  if (ev) hipEventRecord(ev[2], s);
}

// ---- the grouped form: up to MATCH_MAXB problems, one stored query side, stored trains (engine_reps_bin.hip) ------------------------

// Every problem is cut as hamming_geometry(n1, n2, W, 0) cuts it alone, whatever shares the launch; problems without trains are
// left out (prob[k] = the caller's index of table problem k).  Returns the splits of the whole group.
int hamming_group_geometry(int n1, const int *n2, int G, int W, HamGroup &g, int *prob) {
  g = HamGroup();
  g.WK = hamming_kernel_width(W);
  g.tile = HAM_TILE_DWORDS / g.WK;
  g.gx = std::max(1, (n1 + 255) / 256);
  int first = 0;
  for (int i = 0; i < G; i++) {
    if (n2[i] <= 0) continue;
    const HammingGeo one = hamming_geometry(n1, n2[i], W, 0);
    const int p = g.np++;
    prob[p] = i;
    g.n2[p] = n2[i]; g.ntiles[p] = one.ntiles; g.tps[p] = one.tilesPerSplit; g.S[p] = one.S;
    g.first[p] = first;
    first += one.S;
  }
  for (int p = g.np; p <= MATCH_MAXB; p++) g.first[p] = first;
  return first;
}

// part: [splits of the group][n1][2] keys.  Workgroup (x, y) sweeps split y -- whole tiles of ONE problem -- for the queries of
// block x; the keys carry the problem's own train index
template <int WK>
__global__ __launch_bounds__(256, 8) void k_hamg_2nn(const uint32_t *__restrict__ queries, int n1, const HamGroup g,
                                                  unsigned long long *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[HAM_TILE_DWORDS];
  const int q = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const int p = group_problem(g.first, y);
  const int tps = group_pick(g.tps, p);
  const int t0 = (y - group_pick(g.first, p)) * tps, t1 = min(group_pick(g.ntiles, p), t0 + tps);
  unsigned k1, k2;
  ham_sweep<WK>(queries, q, n1, reinterpret_cast<const uint4 *>(group_pick(g.trains, p)), group_pick(g.n2, p), t0, t1, tile, k1, k2);
  if (q < n1) {
    unsigned long long *o = part + ((size_t)y * n1 + q) * 2;
    o[0] = ham_key64(k1);
    o[1] = ham_key64(k2);
  }
}

// nn2[p][q] = {first, d(first), second, d(second)} of query q over the splits of problem p = blockIdx.y
__global__ __launch_bounds__(256) void k_hamg_merge(const unsigned long long *__restrict__ part, int n1, const HamGroup g,
                                                    int4 *__restrict__ nn2) {
  const int q = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
  if (q >= n1) return;
  const int s0 = group_pick(g.first, p);
  ham_merge_splits(part, n1, q, s0, s0 + group_pick(g.S, p), nn2 + ((size_t)p * n1 + q));
}

template <int WK>
static void launch_group_2nn(hipStream_t s, const HamGroup &g, const uint32_t *q, int n1, unsigned long long *part) {
  hipLaunchKernelGGL(k_hamg_2nn<WK>, dim3(g.gx, g.first[g.np]), dim3(256), 0, s, q, n1, g, part);
}

// queries: n1 stored rows of g.WK dwords; g.trains[p]: problem p's stored rows (whole tiles, zero behind n2[p]); part:
// [g.first[g.np]][n1][2] keys; nn2: [g.np][n1] int4.  n1 >= 1, g.np >= 1
void launch_hamming_group(hipStream_t s, const HamGroup &g, const uint32_t *queries, int n1, unsigned long long *part, int *nn2) {
  switch (g.WK) {
    case 1: launch_group_2nn<1>(s, g, queries, n1, part); break;
    case 2: launch_group_2nn<2>(s, g, queries, n1, part); break;
    case 4: launch_group_2nn<4>(s, g, queries, n1, part); break;
    case 8: launch_group_2nn<8>(s, g, queries, n1, part); break;
    default: launch_group_2nn<16>(s, g, queries, n1, part); break;
  }
  hipLaunchKernelGGL(k_hamg_merge, dim3(g.gx, g.np), dim3(256), 0, s, part, n1, g, (int4 *)nn2);
}

// dst: n rows of WK dwords at their place in a stored class (k_hamming_pack on a destination offset; nothing behind them is written)
void launch_hamming_pack_rows(hipStream_t s, const uint8_t *src, int n, int nbytes, int WK, uint32_t *dst) {
  hipLaunchKernelGGL(k_hamming_pack, dim3((unsigned)(((size_t)n * WK + 255) / 256)), dim3(256), 0, s, src, n, nbytes, WK, n, dst);
}

}  // namespace mx
