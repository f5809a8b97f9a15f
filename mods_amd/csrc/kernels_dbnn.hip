// kernels_dbnn.hip -- exact 1-nearest-neighbour distance of selected queries against a resident descriptor database.
//
// Reference: MatchFlannFGINNPlusDB (matching/matching.cpp:462-572).  Its only use of the database is
//   ratioDB = distsRow[0] / distsDB[0]: the squared L2 distance of a query to its NEAREST database descriptor -- never an
// index, so ties do not matter -- and only for queries whose walk produced a record.  The reference asks a kd-tree; here it
// is the matcher's int8 contraction with a plain `min` epilogue, exact: descriptors hold the integers 0..255, so
//   |a-b|^2 - |a-128|^2 = c + 2 a''.b',   a'' = 127 - a,  b' = b - 128,  c = |b'|^2 + 2 sum b'      (kernels_match.hip)
//
// Layout choice: the database is packed ONCE, at creation, into the matcher's operand form WITH the parity partition:
//   rows as int8 b' in 4 KB tiles of 32 rows (16-byte slots XOR-swizzled as k_match_pack writes them), the row constant
//   h = c >> 1 next to them, rows of even c first, then rows of odd c, each class padded to whole stages of TPS tiles with
//   rows that can never win (zero row, h = NONE_H).  The MFMA chain starts from h, an accumulator element is t = h + a''.b',
//   and d - |a'|^2 = 2 t + p with p the class of the TILE: one v_lshl_add per chain instead of one per element.  The final
//   minimum is over both classes.  The host knows the class sizes when it packs (it validates every value anyway), so the
//   regions are contiguous and the geometry (TEp, ntiles) is a launch argument.
//
//   k_db_pack    raw [n][128] u8 -> tiles + row constants, 256 rows per workgroup; the slot bases of a workgroup's two
//                classes come from the host's prefix over the per-workgroup class counts (order inside a class = row order)
//   k_db_select  the matcher's MatchRows -> compacted list of the queries that give a record (the predicate of
//                rows_to_tentatives), its count, and dDB[q] = BIG for every query
//   k_dbnn_min   database rows are the MFMA rows, the selected queries the columns (v_mfma_i32_32x32x32_i8 over K = 128, the
//                sweep core of match_core.hpp: four tiles per barrier through LDS by direct global->LDS loads).  Epilogue per
//                chain: v_min3 tree over the lane's 16 accumulators (8), key 2 t + p (1), v_min into the lane's running
//                minimum (1).  No top-K, no row index.  The number of selected queries is only known on the device: a fixed
//                grid of workgroups is dealt out as (query block, database split) from the device-side count, as
//                k_match_resolve does, so that a few thousand queries fill the machine; the partial minima of the splits
//                meet in one 32-bit integer atomicMin per query -- order-free, hence deterministic.
#undef SWEEP_PHASE_TRACE          // the phase trace of match_core.hpp belongs to kernels_match.hip
#include "match_core.hpp"

namespace mx {

constexpr int DB_PB = 256;                 // database rows per workgroup of k_db_pack
constexpr int DBNN_QS = 2;                 // 32-query sets per wave: 256 queries per 256-thread workgroup
// Workgroups per CU: the sweep core with this epilogue takes 184 VGPRs when the allocator is free; held to the 168 of three
// wavefronts per SIMD it spills the LDS address registers to scratch (68 bytes per lane), so the kernel is built for two.
constexpr int DBNN_WPS = 2;
constexpr int DBNN_NW = 256 * DBNN_WPS;    // workgroups of one round

// the two class regions of n rows with nOdd rows of odd c: tiles of each (multiples of TPS)
DbGeo db_geo(long n, long nOdd) {
  DbGeo g;
  g.TEp = (int)((((n - nOdd + 31) >> 5) + TPS - 1) & ~(long)(TPS - 1));
  g.TOp = (int)((((nOdd + 31) >> 5) + TPS - 1) & ~(long)(TPS - 1));
  return g;
}
size_t db_tiles_bytes(const DbGeo &g) { return (size_t)(g.TEp + g.TOp) * TILE_B; }
size_t db_hrow_bytes(const DbGeo &g) { return (size_t)(g.TEp + g.TOp) * 32 * 4; }
int db_pack_blocks(long n) { return (int)((n + DB_PB - 1) / DB_PB); }

MX_D int sum8x(int v) {                    // sum over the eight lanes that share a row
  v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
  return v;
}

// Eight lanes per row (one 16-byte slice each), 32 rows per pass, 8 passes.  base[blk] = first slot of the workgroup's even
// rows (x) and of its odd rows (y); a row's slot = base of its class + its rank among the workgroup's rows of that class.
__global__ __launch_bounds__(DB_PB) void k_db_pack(const uint8_t *raw, int n, const int2 *base, int totE, int totO, DbGeo geo,
                                                   unsigned char *tiles, int *hrow) {
  __shared__ int sPar[DB_PB], sH[DB_PB], sSlot[DB_PB], sWave[2][4];
  const int tid = threadIdx.x, blk = blockIdx.x, slice = tid & 7, wave = tid >> 6, lane = tid & 63;
  constexpr int NP = DB_PB / 32;
  v4i row[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int t = blk * DB_PB + p * 32 + (tid >> 3);
    row[p] = (v4i){(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
    if (t < n) row[p] = reinterpret_cast<const v4i *>(raw + (size_t)t * 128)[slice];
  }
#pragma unroll
  for (int p = 0; p < NP; p++) {
    v4i v = row[p];
    int s = 0, lin = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      v[w] ^= 0x80808080;                  // b' = b - 128
      s = __builtin_amdgcn_sdot4(v[w], v[w], s, false);
      lin = __builtin_amdgcn_sdot4(v[w], 0x01010101, lin, false);
    }
    row[p] = v;
    s = sum8x(s); lin = sum8x(lin);
    if (slice == 0) { sPar[p * 32 + (tid >> 3)] = lin & 1; sH[p * 32 + (tid >> 3)] = (s + 2 * lin) >> 1; }
  }
  __syncthreads();
  // thread r owns row r of the workgroup: its rank among the rows of its class
  const bool valid = blk * DB_PB + tid < n;
  const int par = sPar[tid];
  const unsigned long long balE = __ballot(valid && !par), balO = __ballot(valid && par);
  const unsigned long long below = (1ull << lane) - 1;
  if (lane == 0) { sWave[0][wave] = __popcll(balE); sWave[1][wave] = __popcll(balO); }
  __syncthreads();
  int rank = par ? __popcll(balO & below) : __popcll(balE & below);
  for (int w = 0; w < wave; w++) rank += sWave[par][w];
  const int2 b = base[blk];
  const int slot = (par ? b.y : b.x) + rank;
  sSlot[tid] = valid ? slot : -1;
  if (valid) hrow[slot] = sH[tid];
  __syncthreads();
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int sl = sSlot[p * 32 + (tid >> 3)];
    if (sl < 0) continue;
    const int tile = sl >> 5, r = sl & 31, sw = (r >> 1) & 7;
    *reinterpret_cast<v4i *>(tiles + (size_t)tile * TILE_B + r * 128 + ((slice ^ sw) << 4)) = row[p];
  }
  if (blk == (int)gridDim.x - 1) {
    // padding rows of both classes: at most 2 * (TPS * 32 - 1) + 62 slots
    const int padE = geo.TEp * 32 - totE, npad = padE + geo.TOp * 32 - totO;
    for (int k = tid >> 3; k < npad; k += 32) {
      const int sl = k < padE ? totE + k : geo.TEp * 32 + totO + (k - padE);
      *reinterpret_cast<v4i *>(tiles + (size_t)(sl >> 5) * TILE_B + (sl & 31) * 128 + (slice << 4)) = (v4i){0, 0, 0, 0};
      if (slice == 0) hrow[sl] = NONE_H;
    }
  }
}

// ---- select -----------------------------------------------------------------------------------------------------------------
struct DbnnProblem {
  const uint8_t *d1;      // [n1][128] u8 queries
  const MatchRow *rows;   // the matcher's result rows; nullptr: every query is selected (the stage tap)
  int *sel, *cnt, *dmin;  // compacted query indices, their number, dDB per QUERY (BIG: not selected)
  int n1, pad;
};
struct DbnnBatch { DbnnProblem p[MATCH_MAXB]; };

// cnt must be 0 at launch.  One global atomic per wave; the order of the list is free (dmin is indexed by query).
__global__ __launch_bounds__(256) void k_db_select(DbnnBatch b, int nn, int allPoints) {
  const DbnnProblem &P = b.p[blockIdx.z];
  const int q = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  bool take = false;
  if (q < P.n1) {
    P.dmin[q] = BIG;
    if (!P.rows) take = true;
    else {
      const MatchRow r = P.rows[q];
      take = r.t0 >= 0 && r.tj >= 0 && (allPoints || (r.nbad == 0 && r.nless <= nn - 2));
    }
  }
  const unsigned long long bal = __ballot(take);
  if (!bal) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(P.cnt, __popcll(bal));
  base = __shfl(base, 0);
  if (take) P.sel[base + __popcll(bal & ((1ull << lane) - 1))] = q;
}

// ---- the 1-NN sweep ------------------------------------------------------------------------------------------------------------
// the NW workgroups of a fixed launch as (query block, split), from the device-side count; a split is whole stages of TPS tiles
struct DbnnGeom { int nQB, S, tilesPerSplit; };
MX_HD DbnnGeom dbnn_geom(int nSel, int ntiles) {
  DbnnGeom G;
  const int QPB = qpb_of(DBNN_QS);
  G.nQB = (nSel + QPB - 1) / QPB;
  int S = G.nQB > 0 ? DBNN_NW / G.nQB : 1;
  if (S > ntiles / MINT) S = ntiles / MINT;
  if (S < 1) S = 1;
  int tps = (ntiles + S - 1) / S;
  tps = (tps + TPS - 1) & ~(TPS - 1);
  S = (ntiles + tps - 1) / tps;
  G.S = S < 1 ? 1 : S;
  G.tilesPerSplit = tps;
  return G;
}
// 8 (v_min3 tree) + 1 (key) + 1 (min) vector instructions per chain
struct MinEpi {
  static constexpr int CH = 1 << 30;       // no index chunks: a key carries no tile number
  int m[DBNN_QS];
  int TEp;
  MX_D int kv(int v) const { return (int)((unsigned)(TEp - 1 - v) >> 31); }   // the tile's parity class: 1 from tile TEp on (scalar arithmetic)
  MX_D void chain(const v16i &acc, int kvv, int s, int) { m[s] = min(m[s], (tree_min16(acc) << 1) + kvv); }
  MX_D void flush(int) {}
};
__global__ __launch_bounds__(256, DBNN_WPS) void k_dbnn_min(DbnnBatch b, const unsigned char *tiles, const int *hrow, int TEp,
                                                                      int ntiles) {
  constexpr int QPB = qpb_of(DBNN_QS);
  __shared__ __attribute__((aligned(16))) unsigned char sm[2][STAGE_B];
  const DbnnProblem &P = b.p[blockIdx.z];
  const int nSel = min(*P.cnt, P.n1);
  const DbnnGeom G = dbnn_geom(nSel, ntiles);
  const int qb = (int)blockIdx.x / G.S, sp = (int)blockIdx.x - qb * G.S;
  if (qb * QPB >= nSel) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, hi = lane >> 5;
  v4i bq[DBNN_QS][4];
  MinEpi epi;
  const int i0 = qb * QPB + wave * (32 * DBNN_QS) + col;      // this lane's place in the list, query set 0
#pragma unroll
  for (int s = 0; s < DBNN_QS; s++) {
    const int q = P.sel[min(i0 + 32 * s, nSel - 1)];
#pragma unroll
    for (int kb = 0; kb < 4; kb++) bq[s][kb] = load_q(P.d1, q, kb, hi);
    epi.m[s] = BIG;
  }
  epi.TEp = TEp;
  const int tBeg = sp * G.tilesPerSplit, tEnd = min(tBeg + G.tilesPerSplit, ntiles);
  sweep_core<DBNN_QS, 10, 4, 1>(tiles, hrow, TEp, TEp, tBeg, tEnd, bq, sm, epi);
#pragma unroll
  for (int s = 0; s < DBNN_QS; s++) {
    // |a - 128|^2 of the lane's half of the row, read again here (the fragments' registers end with the sweep): ~(a ^ 0x7f) = a - 128 as int8
    const int i = i0 + 32 * s, q = P.sel[min(i, nSel - 1)];
    int na = 0;
#pragma unroll
    for (int kb = 0; kb < 4; kb++) {
      const v4i v = load_q(P.d1, q, kb, hi);
#pragma unroll
      for (int w = 0; w < 4; w++) na = __builtin_amdgcn_sdot4(~v[w], ~v[w], na, false);
    }
    na += __shfl_xor(na, 32);
    const int m = min(epi.m[s], __shfl_xor(epi.m[s], 32));     // the 16 + 16 rows of the two lane halves
    if (hi == 0 && i < nSel && m < (NONE_H << 1)) atomicMin(P.dmin + q, m + na);
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
void launch_db_pack(hipStream_t s, const uint8_t *raw, long n, const int2 *base, long nOdd, const DbGeo &geo, unsigned char *tiles,
                    int *hrow) {
  hipLaunchKernelGGL(k_db_pack, dim3(db_pack_blocks(n)), dim3(DB_PB), 0, s, raw, (int)n, base, (int)(n - nOdd), (int)nOdd, geo, tiles, hrow);
}
// sel[i] / dmin[i]: n1[i] ints each; cnt: nb ints, set to zero here.  rows[i] == nullptr selects every query of problem i.
void launch_db_select(hipStream_t s, int nb, const MatchRow *const *rows, const int *n1, int nn, bool allPoints, int *const *sel, int *cnt,
                      int *const *dmin) {
  DbnnBatch b;
  memset(&b, 0, sizeof b);
  int maxN1 = 0;
  for (int i = 0; i < nb; i++) {
    b.p[i].rows = rows ? rows[i] : nullptr; b.p[i].sel = sel[i]; b.p[i].cnt = cnt + i; b.p[i].dmin = dmin[i]; b.p[i].n1 = n1[i];
    maxN1 = std::max(maxN1, n1[i]);
  }
  (void)hipMemsetAsync(cnt, 0, (size_t)nb * 4, s);
  hipLaunchKernelGGL(k_db_select, dim3((maxN1 + 255) / 256, 1, nb), dim3(256), 0, s, b, nn, allPoints ? 1 : 0);
}
void launch_dbnn_min(hipStream_t s, int nb, const uint8_t *const *d1, const int *n1, int *const *sel, int *cnt, int *const *dmin,
                     const DbSet &db) {
  DbnnBatch b;
  memset(&b, 0, sizeof b);
  int maxN1 = 0;
  for (int i = 0; i < nb; i++) {
    b.p[i].d1 = d1[i]; b.p[i].sel = sel[i]; b.p[i].cnt = cnt + i; b.p[i].dmin = dmin[i]; b.p[i].n1 = n1[i];
    maxN1 = std::max(maxN1, n1[i]);
  }
  // one round of workgroups; more only if there could be more query blocks than that
  const int QPB = qpb_of(DBNN_QS);
  hipLaunchKernelGGL(k_dbnn_min, dim3(std::max(DBNN_NW, (maxN1 + QPB - 1) / QPB), 1, nb), dim3(256), 0, s, b, db.tiles, db.hrow, db.geo.TEp,
                     db.geo.TEp + db.geo.TOp);
}

}  // namespace mx
