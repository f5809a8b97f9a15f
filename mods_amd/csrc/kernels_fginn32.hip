// kernels_fginn32.hip -- the exact search of MatchFlannFGINN (matching/matching.cpp:357-461, vector_matcher = linear) on f32 rows of
// any width dim (dim % 4 == 0, 4 <= dim <= MODSX_FGINN32_MAX_DIM) for gfx950.  Nothing of kernels_match.hip / match_core.hpp is used.
//
// Contract (include/modsx.h holds the caller's side):
//   distance  one f32 chain per (query, train) over k = 0, 4, 8, ...: e_i = a[k+i] - b[k+i],
//             r = r + (((e0*e0 + e1*e1) + e2*e2) + e3*e3), every operation rounded to f32, no FMA (-ffp-contract=off), subnormals kept
//             (the default kernel mode): oracle_match.cpp knn_linear.  The f32 MFMA is an fmaf chain and cannot be used: VALU work.
//   order     neighbours by (distance, train index).  Distances are >= +0 and never NaN, so the u32 pattern of the f32 orders like the
//             value and key = (bits << 32) | index is unique per train: min / top-K updates on keys need no visiting order, no tie rule.
//   result    a pure function of the inputs: not of the tile length, the split count, launch order or contexts in flight (integer
//             min / add only, also where atomics merge the splits).
//
// Layout.  k_f32_pack turns dense [n][dim] f32 rows of any 4-byte alignment into rows of DK floats (dim rounded up to the kernel
// width DK in {32, 64, 128, 192, 256}), zero-filled (a zero column adds +0 to every group sum), 16-byte aligned, the train side
// padded with zero rows to whole tiles; it also holds the validity check of the device entry (finite, |x| <= 1e17 -> a flag word).
// Every sweep kernel runs f32_sweep<DK>: one query per lane, 256-thread workgroups, trains staged through LDS in tiles of
// T = 128 / 64 / 32 / 16 / 16 trains (16 KiB; 12 KiB at DK = 192), the next tile fetched into registers while this one is swept;
// every lane reads the same train words (broadcast ds_read_b128, no bank conflicts).  Up to DK = 128 the query row lives in VGPRs.
// At DK = 192 / 256 it is taken in TWO REGISTER CHUNKS of 96 / 128 floats: per tile the lane loads chunk 0, runs the first half of
// every train's chain and parks the partial sum in LDS (T x 256 floats, own-lane slots, no barrier), loads chunk 1 and finishes
// the chains -- the chain order of a pair is unchanged.
//   k_f32_topk<DK>     per query the K = 4 smallest keys of a split (four-deep min / max insertion behind one compare with the
//                      fourth key); the train axis is cut into S splits of whole tiles over gridDim.y
//   k_f32_merge        the 4 smallest of a query's 4 S keys; 32 bytes per query go to the host, which walks j = 1..3
//   k_f32_resolve<DK>  for the queries whose walk is still open: among trains with key > K_last the smallest key of a terminal train
//                      (d >= d_pass, or farther than contradDist from train t0 in f64) and the count of non-terminal ones
// There is no third, rank-counting sweep: it could never change a result.  A terminal train that passes the ratio test has
// d >= d_pass, every non-terminal train has d < d_pass and so a smaller key: the terminal's rank is exactly 3 + count + 1.  A terminal
// train that does not pass gives no record whether the walk reaches it or runs out of its nn first.
// Geometry comes from fginn32_geometry(n1, n2, dim, splits) alone; the cut of the train axis is split_rule (engine.hpp), the one
// rule of every exact search.
// What these kernels have in common with each other and with kernels_fginn_l1.hip / kernels_hamming.hip is written once, in
// search_dev.hpp: the key and Top4 (the four-deep insertion, guarded in the sweeps, unguarded in the merges, and the four-word
// store), f32_merge_splits (the body of k_f32_merge and k_f32g_merge over a split range), F32Resolve (the default or loaded F32Open,
// the anchor position, the per-train step with the terminal rule, the atomic commit: the body of every resolve kernel around its
// own sweep call), group_pick / group_problem (the grouped kernels' table selection).  A kernel here keeps its way to its rows,
// trains, tile range and output, and its sweep call.
//
// Compiler figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; regenerated with the shared pieces in
// place: every figure is what it was, and so is the ISA of every kernel but the two merges):
//   kernel                VGPRs  SGPRs  LDS [B]  scratch  occupancy [waves/SIMD]
//   k_f32_topk<32>           82     24    16384        0      5
//   k_f32_topk<64>          113     24    16384        0      4
//   k_f32_topk<128>         174     24    16384        0      2
//   k_f32_topk<192>         144     26    28672        0      3
//   k_f32_topk<256>         180     27    32768        0      2
//   k_f32_resolve<32>        84     34    16384        0      5
//   k_f32_resolve<64>       114     34    16384        0      4
//   k_f32_resolve<128>      254     34    16384        0      2
//   k_f32_resolve<192>      146     38    28672        0      3
//   k_f32_resolve<256>      182     38    32768        0      2
//   k_f32_pack               14     24        0        0      8
//   k_f32_merge              26     22        0        0      8
//   k_f32g_topk<32>          82     26    16384        0      5
//   k_f32g_topk<64>         113     26    16384        0      4
//   k_f32g_topk<128>        174     26    16384        0      2
//   k_f32g_topk<192>        144     28    28672        0      3
//   k_f32g_topk<256>        180     27    32768        0      2
//   k_f32g_resolve<32>       84     34    16384        0      5
//   k_f32g_resolve<64>      114     34    16384        0      4
//   k_f32g_resolve<128>     254     34    16384        0      2
//   k_f32g_resolve<192>     147     34    28672        0      3
//   k_f32g_resolve<256>     184     34    32768        0      2
//   k_f32g_merge             26     25        0        0      8
// The k_f32g_* kernels are the grouped form (stored representations, engine_reps_f32.hip): the same f32_sweep<DK> body, with the
// problem of a workgroup, its trains and its tile range selected from a by-value table of at most four problems (F32Group) by
// group_problem / group_pick.  The selection is scalar compares on constant indices: it adds SGPRs, no VGPR at DK <= 128, and nothing inside the sweep loop.
// Per (query, train) the sweep loop of k_f32_topk<DK> issues 100 / 195 / 387 / 551 / 744 vector instructions at DK = 32 / 64 / 128 /
// 192 / 256 and DK / 4 ds_read_b128; at DK = 128 that is 96 v_sub_f32, 96 v_mul_f32, 103 v_add_f32, 28 v_pk_add_f32, 16 v_pk_mul_f32
// and 48 for the key and its branch-free insertion (measured times 9.9).
//
// The distance is a template parameter of f32_chain / f32_sweep / k_f32_topk / k_f32_resolve (DIST = MODSX_DIST_L2 by default, or
// MODSX_DIST_L1: vector_dist = L1, r = r + (((|e0| + |e1|) + |e2|) + |e3|), FLANN's L1<float>).  Everything else --
// packing (a zero column adds +0 under L1 too), keys, merge, geometry, the host walk, d_pass and the resolve round trip -- is shared.
// With the parameter in place the ISA of every L2 kernel of this file, k_f32_topk<128> and k_f32_resolve<128> among them, is
// instruction for instruction what it was without it (--save-temps of both, compared per kernel; only the mangled names differ:
// ...ILi128ELi0EE for ...ILi128EE), and the grouped k_f32g_* kernels compile to the same code too.  The L1 instantiations:
//   kernel                VGPRs  SGPRs  LDS [B]  scratch  occupancy [waves/SIMD]
//   k_f32_topk<32, L1>       82     24    16384        0      5
//   k_f32_topk<64, L1>      113     24    16384        0      4
//   k_f32_topk<128, L1>     174     24    16384        0      2
//   k_f32_topk<192, L1>     144     26    28672        0      3
//   k_f32_topk<256, L1>     180     27    32768        0      2
//   k_f32_resolve<32, L1>    84     34    16384        0      5
//   k_f32_resolve<64, L1>   114     34    16384        0      4
//   k_f32_resolve<128, L1>  252     34    16384        0      2
//   k_f32_resolve<192, L1>  146     38    28672        0      3
//   k_f32_resolve<256, L1>  182     38    32768        0      2
// Per (query, train) the sweep loop of k_f32_topk<DK, L1> issues 116 / 179 / 307 / 478 / 606 vector instructions, counted as above; at
// DK = 128: 96 v_sub_f32, 103 v_add_f32 (72 of them with an |x| source modifier), 28 v_pk_add_f32 -- which has no such modifier, so
// 32 v_and_b32 clear sign bits for it -- and 48 for the key and its insertion.  8.1 per group of four against the 8 of the source.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "engine.hpp"
#include "search_dev.hpp"

namespace mx {

int fginn32_kernel_width(int dim) { return dim <= 32 ? 32 : dim <= 64 ? 64 : dim <= 128 ? 128 : dim <= 192 ? 192 : 256; }
static constexpr int f32_tile_trains(int DK) { return DK <= 32 ? 128 : DK <= 64 ? 64 : DK <= 128 ? 32 : 16; }

// splits = 0: production; splits > 0: that many, at most one per tile (split_rule, engine.hpp)
Fginn32Geo fginn32_geometry(int n1, int n2, int dim, int splits) {
  const int DK = fginn32_kernel_width(dim);
  return fginn32_geometry_rows(n1, n2, dim, DK, f32_tile_trains(DK), splits);
}
// the same rule for packed rows of DK dwords staged `tile` at a time (kernels_fginn_l1.hip: its byte rows)
Fginn32Geo fginn32_geometry_rows(int n1, int n2, int dim, int DK, int tile, int splits) {
  Fginn32Geo g;
  g.dim = dim;
  g.DK = DK;
  g.tile = tile;
  g.ntiles = std::max(1, (n2 + g.tile - 1) / g.tile);
  g.gx = std::max(1, (n1 + 255) / 256);
  const SplitCut cut = split_rule(g.ntiles, g.gx, splits);
  g.tilesPerSplit = cut.tilesPerSplit;
  g.S = cut.S;
  return g;
}

static size_t f32_query_bytes(const Fginn32Geo &g) { return (size_t)g.gx * 256 * g.DK * 4; }
static size_t f32_train_bytes(const Fginn32Geo &g) { return (size_t)g.ntiles * g.tile * g.DK * 4; }
// packed queries | packed trains | split keys [S][n1][4] | undecided list [n1] | its results [n1]
size_t fginn32_workspace_bytes(const Fginn32Geo &g, int n1) {
  return f32_query_bytes(g) + f32_train_bytes(g) + (size_t)g.S * n1 * 32 + (size_t)n1 * (sizeof(F32Open) + sizeof(F32Closed)) + 256;
}

// dst: rowsPad rows of DK floats; rows >= n and columns >= dim are zero.  dim % 4 == 0.  *flag |= bit when a value is not finite or
// larger than 1e17 in magnitude (the search then runs on whatever it holds -- indices never come from data -- and the host refuses)
__global__ __launch_bounds__(256) void k_f32_pack(const float *__restrict__ src, int n, int dim, int DK, int rowsPad,
                                                  float4 *__restrict__ dst, unsigned *__restrict__ flag, unsigned bit) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int G = DK / 4;
  if (i >= (size_t)rowsPad * G) return;
  const int row = (int)(i / G), k = 4 * (int)(i % G);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row < n && k < dim) {
    const float *p = src + (size_t)row * dim + k;
    v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
    const bool ok = fabs((double)v.x) <= 1e17 && fabs((double)v.y) <= 1e17 && fabs((double)v.z) <= 1e17 && fabs((double)v.w) <= 1e17;
    if (!ok) atomicOr(flag, bit);      // NaN fails every comparison
  }
  dst[i] = v;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int DK> struct F32Cfg {
  static constexpr int T = f32_tile_trains(DK);
  static constexpr int CH = DK <= 128 ? DK : DK / 2;     // floats of the query row held in VGPRs at a time
  static constexpr int NCH = DK / CH;
  static constexpr int NLOAD = T * DK / 1024;            // float4 per thread and tile
  static constexpr int PART = NCH > 1 ? T * 256 : 4;     // parked partial sums
  static_assert(T * DK % 1024 == 0 && CH % 4 == 0 && CH * NCH == DK, "tile shape");
};

// the chain of one (query chunk, train chunk): r continues over CH floats.  DIST = MODSX_DIST_L2: squares; MODSX_DIST_L1: magnitudes
// (FLANN's L1<float>; the sign bit is dropped by a source modifier of the add, so a group costs 4 v_sub_f32 + 4 v_add_f32)
template <int CH, int DIST = MODSX_DIST_L2>
__device__ __forceinline__ float f32_chain(float r, const float (&a)[CH], const float *__restrict__ b) {
#pragma unroll
  for (int k = 0; k < CH; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(b + k);
    const float e0 = a[k] - v.x, e1 = a[k + 1] - v.y, e2 = a[k + 2] - v.z, e3 = a[k + 3] - v.w;
    if constexpr (DIST == MODSX_DIST_L1) r = r + (((__builtin_fabsf(e0) + __builtin_fabsf(e1)) + __builtin_fabsf(e2)) + __builtin_fabsf(e3));
    else r = r + (((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3);
  }
  return r;
}

template <int CH>
__device__ __forceinline__ void f32_load_chunk(float (&a)[CH], const float *__restrict__ row) {
  if (row) {
#pragma unroll
    for (int k = 0; k < CH; k += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(row + k);
      a[k] = v.x; a[k + 1] = v.y; a[k + 2] = v.z; a[k + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CH; k++) a[k] = 0.f;
  }
}

// Sweeps the tiles [tBeg, tEnd) of `trains` (whole tiles; zero rows behind row n2 - 1 are never visited) for this lane's packed query
// row (null: a lane without a query; it still takes part in the staging) and hands consume(distance, train index) every train.
template <int DK, int DIST = MODSX_DIST_L2, class F>
__device__ __forceinline__ void f32_sweep(const float *__restrict__ qrow, const f32x4 *__restrict__ trains, int n2, int tBeg, int tEnd,
                                          float *__restrict__ tile, float *__restrict__ part, F &&consume) {
  using C = F32Cfg<DK>;
  constexpr int T = C::T, CH = C::CH, NL = C::NLOAD, TILE4 = T * DK / 4;
  const int tid = threadIdx.x;
  float a[CH];
  if constexpr (C::NCH == 1) f32_load_chunk<CH>(a, qrow);
  f32x4 nxt[NL];
#pragma unroll
  for (int i = 0; i < NL; i++) nxt[i] = trains[(size_t)tBeg * TILE4 + i * 256 + tid];
  for (int t = tBeg; t < tEnd; t++) {
    __syncthreads();                                   // the previous tile is no longer read
#pragma unroll
    for (int i = 0; i < NL; i++) reinterpret_cast<f32x4 *>(tile)[i * 256 + tid] = nxt[i];
    __syncthreads();
    if (t + 1 < tEnd) {
#pragma unroll
      for (int i = 0; i < NL; i++) nxt[i] = trains[(size_t)(t + 1) * TILE4 + i * 256 + tid];
    }
    const int base = t * T, jn = min(T, n2 - base);
    if constexpr (C::NCH == 1) {
#pragma unroll 1
      for (int j = 0; j < jn; j++) consume(f32_chain<CH, DIST>(0.f, a, tile + j * DK), base + j);
    } else {
      f32_load_chunk<CH>(a, qrow);
#pragma unroll 1
      for (int j = 0; j < jn; j++) part[j * 256 + tid] = f32_chain<CH, DIST>(0.f, a, tile + j * DK);
      f32_load_chunk<CH>(a, qrow ? qrow + CH : nullptr);
#pragma unroll 1
      for (int j = 0; j < jn; j++) consume(f32_chain<CH, DIST>(part[j * 256 + tid], a, tile + j * DK + CH), base + j);
    }
  }
}

#define F32_SWEEP_LDS(DK)                                                      \
  __shared__ __attribute__((aligned(16))) float tile[F32Cfg<DK>::T * DK];      \
  __shared__ float part[F32Cfg<DK>::PART]

// keys: [S][n1][4].  Split blockIdx.y sweeps the tiles [y * tilesPerSplit, ...).
template <int DK, int DIST = MODSX_DIST_L2>
__global__ __launch_bounds__(256) void k_f32_topk(const float *__restrict__ queries, int n1, const float4 *__restrict__ trains, int n2,
                                                  int ntiles, int tilesPerSplit, unsigned long long *__restrict__ keys) {
  F32_SWEEP_LDS(DK);
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int t0 = blockIdx.y * tilesPerSplit, t1 = min(ntiles, t0 + tilesPerSplit);
  Top4 top;
  f32_sweep<DK, DIST>(q < n1 ? queries + (size_t)q * DK : nullptr, reinterpret_cast<const f32x4 *>(trains), n2, t0, t1, tile, part,
                      [&](float d, int idx) { top.put_below(f32_key(d, idx)); });
  if (q < n1) top.store(keys + ((size_t)blockIdx.y * n1 + q) * 4);
}

// top4[q] = the four smallest of the 4 S keys of query q (all ones where there is none)
__global__ __launch_bounds__(256) void k_f32_merge(const unsigned long long *__restrict__ keys, int n1, int S,
                                                   unsigned long long *__restrict__ top4) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n1) return;
  f32_merge_splits(keys, n1, q, 0, S, top4 + (size_t)q * 4);
}

// open[u]: an undecided query; closed[u] (kterm = all ones, cnt = 0 on entry) receives over all splits the smallest key of a terminal
// train and the count of non-terminal trains among the trains with key > klast.  pos: [n2][2] f64.
template <int DK, int DIST = MODSX_DIST_L2>
__global__ __launch_bounds__(256) void k_f32_resolve(const float *__restrict__ queries, const F32Open *__restrict__ open, int nu,
                                                     const float4 *__restrict__ trains, int n2, int ntiles, int tilesPerSplit,
                                                     const double *__restrict__ pos, double contrDistSq, F32Closed *__restrict__ closed) {
  F32_SWEEP_LDS(DK);
  const int u = blockIdx.x * 256 + threadIdx.x;
  const int t0 = blockIdx.y * tilesPerSplit, t1 = min(ntiles, t0 + tilesPerSplit);
  F32Resolve r(open, u, u < nu, pos, contrDistSq);
  f32_sweep<DK, DIST>(u < nu ? queries + (size_t)r.o.q * DK : nullptr, reinterpret_cast<const f32x4 *>(trains), n2, t0, t1, tile, part,
                      [&](float d, int idx) { r.step(d, idx); });
  r.commit(closed, u, u < nu);
}

// the keys of every search in this format merge alike (kernels_fginn_l1.hip launches it too)
void launch_fginn32_merge(hipStream_t s, const Fginn32Geo &g, const unsigned long long *keys, int n1, unsigned long long *top4) {
  hipLaunchKernelGGL(k_f32_merge, dim3(g.gx), dim3(256), 0, s, keys, n1, g.S, top4);
}

Fginn32Work fginn32_work(const Fginn32Geo &g, int n1, void *work) {
  Fginn32Work w;
  char *p = (char *)work;
  w.queries = (float *)p; p += f32_query_bytes(g);
  w.trains = (float *)p; p += f32_train_bytes(g);
  w.keys = (unsigned long long *)p; p += (size_t)g.S * n1 * 32;
  w.open = (F32Open *)p; p += (size_t)n1 * sizeof(F32Open);
  w.closed = (F32Closed *)p;
  return w;
}

template <int DK>
static void launch_topk(hipStream_t s, const Fginn32Geo &g, const Fginn32Work &w, int n1, int n2, int dist) {
  const auto k = dist == MODSX_DIST_L1 ? k_f32_topk<DK, MODSX_DIST_L1> : k_f32_topk<DK>;
  hipLaunchKernelGGL(k, dim3(g.gx, g.S), dim3(256), 0, s, w.queries, n1, (const float4 *)w.trains, n2, g.ntiles, g.tilesPerSplit, w.keys);
}
template <int DK>
static void launch_resolve(hipStream_t s, const Fginn32Geo &g, const Fginn32Work &w, int nu, int n2, const double *pos, double cd2, int dist) {
  const auto k = dist == MODSX_DIST_L1 ? k_f32_resolve<DK, MODSX_DIST_L1> : k_f32_resolve<DK>;
  hipLaunchKernelGGL(k, dim3((nu + 255) / 256, g.S), dim3(256), 0, s, w.queries, w.open, nu, (const float4 *)w.trains, n2, g.ntiles,
                     g.tilesPerSplit, pos, cd2, w.closed);
}
#define F32_BY_WIDTH(g, fn, ...)               \
  switch ((g).DK) {                            \
    case 32: fn<32>(__VA_ARGS__); break;       \
    case 64: fn<64>(__VA_ARGS__); break;       \
    case 128: fn<128>(__VA_ARGS__); break;     \
    case 192: fn<192>(__VA_ARGS__); break;     \
    default: fn<256>(__VA_ARGS__); break;      \
  }

// d1 / d2: dense [n][dim] f32 rows in HBM (4-byte aligned); work: fginn32_workspace_bytes(g, n1), 256-byte aligned; flagAndTop4: 16
// bytes (the validity flag word: bit 0 = queries, bit 1 = trains) followed by n1 x 4 keys.  n1 >= 1, n2 >= 1.  ev (optional): three
// events -- before the packing, between the packing and the search (k_f32_topk + k_f32_merge), behind the search.  dist: MODSX_DIST_L2
// or MODSX_DIST_L1 (checked by the caller); it selects the chain of the sweep and nothing else
void launch_fginn32_topk(hipStream_t s, const Fginn32Geo &g, const float *d1, int n1, const float *d2, int n2, void *work,
                         void *flagAndTop4, hipEvent_t *ev, int dist) {
  const Fginn32Work w = fginn32_work(g, n1, work);
  const int qRows = g.gx * 256, tRows = g.ntiles * g.tile, G = g.DK / 4;
  unsigned *flag = (unsigned *)flagAndTop4;
  hipMemsetAsync(flag, 0, 16, s);
  if (ev) hipEventRecord(ev[0], s);
  hipLaunchKernelGGL(k_f32_pack, dim3((unsigned)(((size_t)qRows * G + 255) / 256)), dim3(256), 0, s, d1, n1, g.dim, g.DK, qRows,
                     (float4 *)w.queries, flag, 1u);
  hipLaunchKernelGGL(k_f32_pack, dim3((unsigned)(((size_t)tRows * G + 255) / 256)), dim3(256), 0, s, d2, n2, g.dim, g.DK, tRows,
                     (float4 *)w.trains, flag, 2u);
  if (ev) hipEventRecord(ev[1], s);
  F32_BY_WIDTH(g, launch_topk, s, g, w, n1, n2, dist);
  launch_fginn32_merge(s, g, w.keys, n1, (unsigned long long *)((char *)flagAndTop4 + 16));
  if (ev) hipEventRecord(ev[2], s);
}

// the packed rows of the last launch_fginn32_topk on this workspace are reused; the caller has set w.open[0 .. nu) and
// w.closed[0 .. nu) = {all ones, 0}
void launch_fginn32_resolve(hipStream_t s, const Fginn32Geo &g, int n1, int nu, int n2, const double *pos, double contrDistSq, void *work,
                            int dist) {
  const Fginn32Work w = fginn32_work(g, n1, work);
  static_assert(sizeof(F32Closed) == 16 && sizeof(F32Open) == 24, "record sizes");
  F32_BY_WIDTH(g, launch_resolve, s, g, w, nu, n2, pos, contrDistSq, dist);
}

// ---- the grouped form: up to MATCH_MAXB problems, one stored query side, stored trains (engine_reps_f32.hip) ----------------------

int fginn32_group_geometry(int n1, const int *n2, int G, int dim, F32Group &g, int *prob) {
  g = F32Group();
  g.DK = fginn32_kernel_width(dim);
  g.tile = f32_tile_trains(g.DK);
  g.gx = std::max(1, (n1 + 255) / 256);
  int first = 0;
  for (int i = 0; i < G; i++) {
    if (n2[i] <= 0) continue;
    const Fginn32Geo one = fginn32_geometry(n1, n2[i], dim, 0);      // every problem is cut as it would be alone
    const int p = g.np++;
    prob[p] = i;
    g.n2[p] = n2[i]; g.ntiles[p] = one.ntiles; g.tps[p] = one.tilesPerSplit; g.S[p] = one.S;
    g.first[p] = first;
    first += one.S;
  }
  for (int p = g.np; p <= MATCH_MAXB; p++) g.first[p] = first;
  return first;
}

// keys: [splits][n1][4].  Workgroup (x, y) sweeps split y -- tiles of ONE problem -- for the queries of block x; train indices are
// the problem's own
template <int DK>
__global__ __launch_bounds__(256) void k_f32g_topk(const float *__restrict__ queries, int n1, const F32Group g,
                                                   unsigned long long *__restrict__ keys) {
  F32_SWEEP_LDS(DK);
  const int q = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const int p = group_problem(g.first, y);
  const int tps = group_pick(g.tps, p), ntiles = group_pick(g.ntiles, p);
  const int t0 = (y - group_pick(g.first, p)) * tps, t1 = min(ntiles, t0 + tps);
  Top4 top;
  f32_sweep<DK>(q < n1 ? queries + (size_t)q * DK : nullptr, reinterpret_cast<const f32x4 *>(group_pick(g.trains, p)), group_pick(g.n2, p),
                t0, t1, tile, part, [&](float d, int idx) { top.put_below(f32_key(d, idx)); });
  if (q < n1) top.store(keys + ((size_t)y * n1 + q) * 4);
}

// top4[p][q] = the four smallest keys of query q over the splits of problem p = blockIdx.y
__global__ __launch_bounds__(256) void k_f32g_merge(const unsigned long long *__restrict__ keys, int n1, const F32Group g,
                                                    unsigned long long *__restrict__ top4) {
  const int q = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
  if (q >= n1) return;
  const int s0 = group_pick(g.first, p);
  f32_merge_splits(keys, n1, q, s0, s0 + group_pick(g.S, p), top4 + ((size_t)p * n1 + q) * 4);
}

// k_f32_resolve for the open walks of every problem at once: workgroup x belongs to one problem, one block of 256 of its open
// entries and one of its splits
template <int DK>
__global__ __launch_bounds__(256) void k_f32g_resolve(const float *__restrict__ queries, const F32Open *__restrict__ open, const F32Group g,
                                                      double contrDistSq, F32Closed *__restrict__ closed) {
  F32_SWEEP_LDS(DK);
  const int x = blockIdx.x;
  const int p = group_problem(g.rfirst, x);
  const int S = group_pick(g.S, p), local = x - group_pick(g.rfirst, p), ub = local / S, sp = local - ub * S;
  const int tps = group_pick(g.tps, p), ntiles = group_pick(g.ntiles, p);
  const int t0 = sp * tps, t1 = min(ntiles, t0 + tps);
  const int u = group_pick(g.ubeg, p) + ub * 256 + threadIdx.x;
  const bool live = u < group_pick(g.uend, p);
  F32Resolve r(open, u, live, group_pick(g.pos, p), contrDistSq);
  f32_sweep<DK>(live ? queries + (size_t)r.o.q * DK : nullptr, reinterpret_cast<const f32x4 *>(group_pick(g.trains, p)), group_pick(g.n2, p),
                t0, t1, tile, part, [&](float d, int idx) { r.step(d, idx); });
  r.commit(closed, u, live);
}

template <int DK>
static void launch_group_topk(hipStream_t s, const F32Group &g, const float *queries, int n1, unsigned long long *keys) {
  hipLaunchKernelGGL(k_f32g_topk<DK>, dim3(g.gx, g.first[g.np]), dim3(256), 0, s, queries, n1, g, keys);
}
template <int DK>
static void launch_group_resolve(hipStream_t s, const F32Group &g, const float *queries, const F32Open *open, double cd2, F32Closed *closed) {
  hipLaunchKernelGGL(k_f32g_resolve<DK>, dim3(g.rfirst[g.np]), dim3(256), 0, s, queries, open, g, cd2, closed);
}

void launch_fginn32_group_topk(hipStream_t s, const F32Group &g, const float *queries, int n1, unsigned long long *keys,
                               unsigned long long *top4) {
  F32_BY_WIDTH(g, launch_group_topk, s, g, queries, n1, keys);
  hipLaunchKernelGGL(k_f32g_merge, dim3(g.gx, g.np), dim3(256), 0, s, keys, n1, g, top4);
}

void launch_fginn32_group_resolve(hipStream_t s, const F32Group &g, const float *queries, const F32Open *open, double contrDistSq,
                                  F32Closed *closed) {
  F32_BY_WIDTH(g, launch_group_resolve, s, g, queries, open, contrDistSq, closed);
}

void launch_fginn32_pack_rows(hipStream_t s, const float *src, int n, int dim, int DK, float *dst, unsigned *flag, unsigned bit) {
  hipLaunchKernelGGL(k_f32_pack, dim3((unsigned)(((size_t)n * (DK / 4) + 255) / 256)), dim3(256), 0, s, src, n, dim, DK, n, (float4 *)dst,
                     flag, bit);
}

}  // namespace mx
