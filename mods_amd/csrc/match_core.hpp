// match_core.hpp -- what the int8 sweeps share: the tile layout k_match_pack writes, the staging of four tiles per barrier
// (direct global -> LDS loads, XOR-swizzled 16-byte slots), and the MFMA core with its epilogue policy.  Used by
// kernels_match.hip (sweep 1, resolve) and kernels_dbnn.hip (the 1-NN pass against a descriptor database).
#pragma once
#include <type_traits>
#include "engine.hpp"

namespace mx {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int BIG = 0x7fffffff;
constexpr int NONE_H = 0x3fffff;           // row constant of a padding row: t = NONE_H + 0
constexpr int NONE_KEY = NONE_H << 9;      // 0x7ffffe00: empty slot of a running minimum; every real key is smaller, every padding key larger
constexpr int TPS = 4;                     // train tiles staged per barrier
constexpr int CHUNK = 240;                 // tiles per index chunk (absolute tile numbers): the low byte of a key is tile % CHUNK + 1
constexpr int MINT = 12;                   // fewest tiles a split is made of

// 32-query sets per wave (QS, even): 2 for most problems -- 3 wavefronts per SIMD --, 4 when both sides hold >= 40 k descriptors:
// every LDS fragment read then feeds four MFMA chains (half the LDS bytes per matrix instruction) at 2 wavefronts per SIMD
constexpr int sweep_wps(int qs) { return qs >= 4 ? 2 : 3; }   // waves per SIMD the sweeps are built for
constexpr int qpb_of(int qs) { return 4 * 32 * qs; }          // queries per 256-thread workgroup (k_match_resolve)

constexpr int TILE_B = 4096;
constexpr int HOFF = TPS * TILE_B, STAGE_B = HOFF + TPS * 128;
constexpr int MAXD = 128 * 255 * 255;      // largest possible squared distance

// Tile geometry of a problem.  Host side: the capacity of one class region (either class may hold every train) and an upper
// bound of the virtual tile count.  Device side (written by k_match_pack's last workgroup): the padded tile counts.
MX_HD int region_tiles(int n2) { return (((n2 + 31) / 32 + TPS - 1) & ~(TPS - 1)) + TPS; }
MX_HD int ntiles_ub(int n2) { return (((n2 + 31) / 32 + TPS - 1) & ~(TPS - 1)) + 2 * TPS; }
struct TileGeo { int TEp, TOp, ntilesV, pad; };   // even / odd class tiles (multiples of TPS), their sum
MX_D int phys_tile(int v, int TEp, int offT) { return v < TEp ? v : offT + v - TEp; }

MX_D bool lex_less(int da, int ia, int db, int ib) { return da < db || (da == db && ia < ib); }
MX_D int imed3(int a, int b, int c) { return min(max(a, b), max(min(a, b), c)); }
MX_D int imin3(int a, int b, int c) { return min(min(a, b), c); }

// Sweep 2 runs over the UNDECIDED queries only, whose number the host does not know at launch time.  Every workgroup of a fixed
// one-round launch therefore derives the split geometry from the device-side count: the NW workgroups are dealt out as
// (query block, split) with as many splits as fill the machine once.
// workgroups of k_match_resolve that hold a (query block, split): one per CU while the undecided queries fill at most two
// blocks (the usual 1-3 %: more workgroups would only wait for LDS), a full round of the sweeps' size beyond that (inputs with
// many near-duplicates per query: shorter splits, fewer logged groups per stream)
MX_HD int resolve_nw(int nQB, int qs) { return nQB <= 2 ? 256 : 256 * sweep_wps(qs); }
struct Sweep2Geom { int nQB, S, tilesPerSplit; };
MX_HD Sweep2Geom sweep2_geom(int nUnd, int ntiles, int qs) {
  Sweep2Geom G;
  const int QPB = qpb_of(qs);
  G.nQB = (nUnd + QPB - 1) / QPB;
  const int SWEEP2_NW = resolve_nw(G.nQB, qs);
  int S = G.nQB > 0 ? SWEEP2_NW / G.nQB : 1;
  if (S > ntiles / MINT) S = ntiles / MINT;
  if (S < 1) S = 1;
  int tps = (ntiles + S - 1) / S;
  tps = (tps + TPS - 1) & ~(TPS - 1);
  S = (ntiles + tps - 1) / tps;
  G.S = S < 1 ? 1 : S;
  G.tilesPerSplit = tps;
  return G;
}
// register r of the 32x32 accumulator of lane half `hi` holds MFMA row 8 (r >> 2) + 4 hi + (r & 3)
MX_D int row_of(int r, int hi) { return 8 * (r >> 2) + 4 * hi + (r & 3); }

// ---------------- staging: 4 tiles + their constants, global -> LDS directly ------------------------------------------
typedef const unsigned char __attribute__((address_space(1))) *gbptr;
typedef unsigned char __attribute__((address_space(3))) *lbptr;
template <int NW>      // wavefronts of the workgroup.  16 chunks of tile bytes (1 KB per wave instruction) + 2 of row constants
MX_D void stage_group(const unsigned char *tiles, const int *hrow, int p0, unsigned char *buf, int wave, int lane) {
  // a producing wavefront takes CPW CONSECUTIVE chunks: one address pair and one M0 for all of them, the instruction's immediate
  // offset (applied to the global and to the LDS address alike) steps through them
  constexpr int CPW = NW >= 8 ? 2 : 4, NPROD = 16 / CPW;
  if (wave < NPROD) {
    const unsigned char *src = tiles + (size_t)p0 * TILE_B + (size_t)wave * (CPW * 1024) + lane * 16;
    unsigned char *dst = buf + wave * (CPW * 1024);
    __builtin_amdgcn_global_load_lds((gbptr)src, (lbptr)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbptr)src, (lbptr)dst, 16, 1024, 0);
    if (CPW == 4) {
      __builtin_amdgcn_global_load_lds((gbptr)src, (lbptr)dst, 16, 2048, 0);
      __builtin_amdgcn_global_load_lds((gbptr)src, (lbptr)dst, 16, 3072, 0);
    }
  }
  const int k = NW - 1 - wave;        // the last two wavefronts bring the row constants
  if (k < 2)
    __builtin_amdgcn_global_load_lds((gbptr)(reinterpret_cast<const unsigned char *>(hrow + (size_t)p0 * 32) + k * 256 + lane * 4),
                                     (lbptr)(buf + HOFF + k * 256), 4, 0, 0);
}
MX_D v4i read_a(const unsigned char *tile, int row, int kb, int hi) {
  const int slot = 2 * kb + hi;
  return *reinterpret_cast<const v4i *>(tile + row * 128 + ((slot ^ ((row >> 1) & 7)) << 4));
}
// the query fragment: a'' = 127 - a = -(a - 128) - 1 (u8 -> i8 by x ^ 0x7f), bytes [32 kb + 16 hi, +16)
MX_D v4i load_q(const uint8_t *base, int row, int kb, int hi) {
  v4i v = *reinterpret_cast<const v4i *>(base + (size_t)row * 128 + 32 * kb + 16 * hi);
  v[0] ^= 0x7f7f7f7f; v[1] ^= 0x7f7f7f7f; v[2] ^= 0x7f7f7f7f; v[3] ^= 0x7f7f7f7f;
  return v;
}
MX_D int tree_min16(const v16i &k) {
  const int t0 = imin3(k[0], k[1], k[2]), t1 = imin3(k[3], k[4], k[5]), t2 = imin3(k[6], k[7], k[8]);
  const int t3 = imin3(k[9], k[10], k[11]), t4 = imin3(k[12], k[13], k[14]);
  return min(imin3(t0, t1, t2), imin3(t3, t4, k[15]));
}

// LDS reads of the sweep core as assembly (the waits are counted by hand there): the four fragment slices of tile Q of a stage,
// and its 16 row constants
template <int Q>
MX_D void lds_load_af(unsigned base, const unsigned (&aAddr)[4], v4i *af) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[0]) : "v"(base + aAddr[0]), "n"(Q * TILE_B));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[1]) : "v"(base + aAddr[1]), "n"(Q * TILE_B));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[2]) : "v"(base + aAddr[2]), "n"(Q * TILE_B));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[3]) : "v"(base + aAddr[3]), "n"(Q * TILE_B));
}
template <int Q>
MX_D void lds_load_c(unsigned addr, v16i &C) {
  v4i c0, c1, c2, c3;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(c0) : "v"(addr), "n"(Q * 128));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(c1) : "v"(addr), "n"(Q * 128 + 32));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(c2) : "v"(addr), "n"(Q * 128 + 64));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(c3) : "v"(addr), "n"(Q * 128 + 96));
  C = __builtin_shufflevector(__builtin_shufflevector(c0, c1, 0, 1, 2, 3, 4, 5, 6, 7), __builtin_shufflevector(c2, c3, 0, 1, 2, 3, 4, 5, 6, 7),
                              0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
}

// ---------------- the sweep core: tiles through LDS, MFMA chains, an epilogue per chain ---------------------------------------
// One instruction stream per wave keeps both pipes busy: while the four MFMAs of a (tile, query set) chain run, the wave
// reduces the accumulators of the previous chain, so the matrix pipe never waits for a whole wave to leave its epilogue.
// Fragments and row constants of the next tile are read from LDS one tile ahead (two register sets).  The epilogue is a policy:
//   int  kv(v)                          the wave-uniform constant of virtual tile v
//   void chain(acc, kv, s, tile)        reduce one accumulator (query set s, virtual tile `tile`)
//   void flush(chunkTile0)              end of an index chunk (CH tiles, absolute tile numbers)
#ifdef SWEEP_PHASE_TRACE
// debugging aid (tools/trace_sweep_phases.py; tools/build_variant.sh ptrace "-DSWEEP_PHASE_TRACE"): per wavefront of the last
// k_match_sweep1 launch, shader-clock cycles spent waiting at the stage barriers / issuing the next stage's DMA / in the tiles, its
// total, stages, and the 100 MHz wall clock at its start and end.  (A stamp is an s_memtime + s_waitcnt: a few hundred cycles each.)
__device__ unsigned long long g_ptrace[16384][8];
#define PTRACE(x) x
#else
#define PTRACE(x)
#endif
// SPB: groups of TPS tiles per barrier.  A workgroup that is alone on its CU (sweep 1) has nobody to cover the bubble at a
// barrier -- every wavefront refills its pipeline at the same moment --, so it stages SPB groups at once and meets 1 / SPB as often.
template <int QSETS, int EPI_VALU, int NW, int SPB, class Epi>
__device__ __forceinline__ void sweep_core(const unsigned char *tiles, const int *hrow, int TEp, int offT, int tBeg, int tEnd,
                                           const v4i (&bq)[QSETS][4], unsigned char (&sm)[2 * SPB][STAGE_B], Epi &epi) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 31, hi = lane >> 5;
  // The LDS reads are written as assembly with the waits counted by hand: the compiler orders every wait behind the reads
  // of the NEXT tile it has just issued (`s_waitcnt lgkmcnt(0)` -- a pending global->LDS load makes it give up counting), which
  // exposed one LDS latency per tile.  Reads issue and return in order, so "all but the newest 4" is exactly "everything of
  // the current tile".  Per-lane addresses: fragment slot 2 kb + hi of row col (swizzled), row constants 16 hi.
  unsigned aAddr[4];
#pragma unroll
  for (int kb = 0; kb < 4; kb++) aAddr[kb] = (unsigned)(col * 128 + (((2 * kb + hi) ^ ((col >> 1) & 7)) << 4));
  const unsigned cAddr = (unsigned)(HOFF + 16 * hi);
  const unsigned smBase = (unsigned)(size_t)(lbptr)&sm[0][0];
  v4i af[2][4];
  v16i C[2];
  int kv[2];
  v16i acc[2];
  // the pipeline starts with a neutral pending chain: keys that change nothing
#pragma unroll
  for (int r = 0; r < 16; r++) acc[1][r] = NONE_H;
  int kvPend = 0, pendTile = 0;
#pragma unroll
  for (int j = 0; j < SPB; j++)
    if (tBeg + j * TPS < tEnd) stage_group<NW>(tiles, hrow, phys_tile(tBeg + j * TPS, TEp, offT), sm[j], wave, lane);
  int it = 0;
  PTRACE(unsigned long long pa0 = 0; unsigned long long pa1 = 0; unsigned long long pa2 = 0; unsigned long long pt0 = __builtin_readcyclecounter(); const unsigned long long pstart = pt0; const unsigned long long pwall = wall_clock64();)
  for (int tb = tBeg; tb < tEnd; tb += TPS * SPB, it++) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PTRACE(const unsigned long long pt1 = __builtin_readcyclecounter();)
#pragma unroll
    for (int j = 0; j < SPB; j++) {
      const int t = tb + TPS * SPB + j * TPS;
      if (t < tEnd) stage_group<NW>(tiles, hrow, phys_tile(t, TEp, offT), sm[((it & 1) ^ 1) * SPB + j], wave, lane);
    }
    PTRACE(const unsigned long long pt2 = __builtin_readcyclecounter(); pa0 += pt1 - pt0; pa1 += pt2 - pt1;)
   for (int j = 0; j < SPB; j++) {
    const int tg = tb + j * TPS;
    if (tg >= tEnd) break;
    const unsigned base = smBase + ((it & 1) * SPB + j) * STAGE_B;
    lds_load_af<0>(base, aAddr, af[0]);
    lds_load_c<0>(base + cAddr, C[0]);
    kv[0] = epi.kv(tg);
    // one tile: phase s = the chain of (tile q, set s) beside the reduction of the previous chain -- (tile q, set s - 1), or the
    // last set of the previous tile.  QSETS is even, so the chains alternate between the two accumulators.  The fragment reads
    // of the NEXT tile are issued in front of phase 0, its row constants in front of phase 1.
    auto tile = [&](auto qc) {
      constexpr int q = decltype(qc)::value, cur = q & 1;
#pragma unroll
      for (int s = 0; s < QSETS; s++) {
        if (q + 1 < TPS) {
          if (s == 0) lds_load_af<(q + 1) % TPS>(base, aAddr, af[cur ^ 1]);
          if (s == 1) { lds_load_c<(q + 1) % TPS>(base + cAddr, C[cur ^ 1]); kv[cur ^ 1] = epi.kv(tg + q + 1); }
        }
        if (s == 0) {
          // everything of THIS tile has landed once at most the reads just issued (4, none in the last tile of a stage) are pending
          if (q + 1 < TPS)
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(af[cur][0]), "+v"(af[cur][1]), "+v"(af[cur][2]), "+v"(af[cur][3]), "+v"(C[cur]));
          else
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[cur][0]), "+v"(af[cur][1]), "+v"(af[cur][2]), "+v"(af[cur][3]), "+v"(C[cur]));
        }
        __builtin_amdgcn_sched_barrier(0);
        v16i &an = acc[s & 1];
        an = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[cur][0], bq[s][0], C[cur], 0, 0, 0);
#pragma unroll
        for (int kb = 1; kb < 4; kb++) an = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[cur][kb], bq[s][kb], an, 0, 0, 0);
        if (s == 0) epi.chain(acc[1], kvPend, QSETS - 1, pendTile);
        else epi.chain(acc[(s - 1) & 1], kv[cur], s - 1, tg + q);
        // one MFMA, then a quarter of the reduction
        constexpr int Q1 = (EPI_VALU + 3) / 4, Q2 = (EPI_VALU + 2) / 4, Q3 = (EPI_VALU + 1) / 4, Q4 = EPI_VALU / 4;
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, Q1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, Q2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, Q3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, Q4, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      pendTile = tg + q;
      kvPend = kv[cur];
    };
    tile(std::integral_constant<int, 0>{});
    tile(std::integral_constant<int, 1>{});
    tile(std::integral_constant<int, 2>{});
    tile(std::integral_constant<int, 3>{});
    static_assert(TPS == 4, "four tiles per stage");
    if ((tg + TPS) % Epi::CH == 0) {
      // end of an index chunk: drain the pending chain, then move the indices of new keys out of the low byte
      epi.chain(acc[1], kvPend, QSETS - 1, pendTile);
#pragma unroll
      for (int r = 0; r < 16; r++) acc[1][r] = NONE_H;
      kvPend = 0;
      epi.flush(tg + TPS - Epi::CH);
    }
   }
   PTRACE({ const unsigned long long pt3 = __builtin_readcyclecounter(); pa2 += pt3 - pt2; pt0 = pt3; })
  }
  if (tEnd > tBeg && tEnd % Epi::CH) {
    epi.chain(acc[1], kvPend, QSETS - 1, pendTile);
    epi.flush((tEnd / Epi::CH) * Epi::CH);
  }
#ifdef SWEEP_PHASE_TRACE
  if (Epi::CH == CHUNK && lane == 0) {       // sweep 1 only (k_match_resolve runs the same core)
    const int wg = blockIdx.x + gridDim.x * blockIdx.y;
    if (wg * NW + wave < 16384) {
      unsigned long long *o = g_ptrace[wg * NW + wave];
      o[0] = pa0; o[1] = pa1; o[2] = pa2; o[3] = __builtin_readcyclecounter() - pstart; o[4] = (unsigned long long)it * SPB; o[5] = wall_clock64();
      o[6] = (unsigned long long)QSETS; o[7] = pwall;
    }
  }
#endif
}

}  // namespace mx
