// kernels_liop.hip -- the LIOP descriptor of a normalised 41 x 41 patch.
//
// Reference: LIOPDescriptor::operator()   matching/liopdesc.hpp:55-63
//   vl_liopdesc_new_basic / vl_liopdesc_new   vlfeat/vl/liop.c:320-411  (4 neighbours, 6 spatial bins, radius 6, threshold -(5/255))
//   vl_liopdesc_process                       vlfeat/vl/liop.c:440-555
//   patch_sort / neigh_sort                   vlfeat/vl/qsort-def.h:126-165 (pivot (begin + end) / 2 to the end, Lomuto scan, cmp <= 0)
// One 256-thread workgroup per patch.  The 673 measurement pixels are sorted by intensity in LDS (bitonic, 64-bit keys
// intensity | index: a STABLE order).  The six spatial bins are cut by rank, so the order inside a group of equal intensities
// matters only when such a group lies across one of the five cuts (ranks 112 k): then -- and only then -- lane 0 replays the
// reference's quicksort on the identity permutation; otherwise any order by key gives the reference's histogram (a bin adds
// small integers, exact in f32 in any order).  The replay knows the sorted keys, so a partition whose pivot is its segment's
// maximum (everything <= pivot: the scan swaps every element with itself) is taken in one step; that is what makes a constant
// disc cost 673 steps instead of 226 k.
// Per pixel, by rank: four bilinear samples in f64 from the table the host built with libm (engine_liop.hip), the reference's
// quicksort on the four, the lexicographic index of that permutation, the weight, one LDS integer add.  Intensities are compared,
// never subtracted (a - b <= 0 is a <= b only under gradual underflow); -0 ties with +0; non-finite patch values are outside
// the contract.
#include "engine.hpp"

namespace mx {

constexpr int LP_SIDE = 41, LP_NPX = LP_SIDE * LP_SIDE, LP_N = MODSX_LIOP_PIXELS, LP_BINS = 6, LP_AREA = LP_N / LP_BINS, LP_DIM = MODSX_LIOP_DIM;
constexpr int LP_SORT = 1024, LP_T = 256, LP_STACK = 32;
static_assert(LP_N <= LP_SORT && LP_DIM == 24 * LP_BINS && LP_AREA == 112, "vl_liopdesc_new_basic(41)");

// --- the reference's quicksort on four values, the permutation packed into nibbles (no indexed private arrays) ---
MX_D float lp_val(const float (&v)[4], unsigned j) { return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3])); }
MX_D unsigned lp_get(unsigned p, int i) { return (p >> (4 * i)) & 3u; }
MX_D unsigned lp_swap(unsigned p, int i, int j) {
  const unsigned a = lp_get(p, i), b = lp_get(p, j);
  p &= ~((15u << (4 * i)) | (15u << (4 * j)));
  return p | (b << (4 * i)) | (a << (4 * j));      // i == j: a == b
}
MX_D int lp_partition(unsigned &p, const float (&v)[4], int b, int e) {
  p = lp_swap(p, (b + e) >> 1, e);
  const float kp = lp_val(v, lp_get(p, e));
  int lo = b;
  for (int i = b; i < e; i++)
    if (lp_val(v, lp_get(p, i)) <= kp) { p = lp_swap(p, lo, i); lo++; }
  p = lp_swap(p, lo, e);
  return lo;
}
template <int D>
MX_D void lp_qsort4(unsigned &p, const float (&v)[4], int b, int e) {   // D partitions deep: 4 -> <= 3 -> <= 2 -> <= 1 elements
  if constexpr (D > 0) {
    if (b >= e) return;                                                  // one element: the reference swaps it with itself
    const int lo = lp_partition(p, v, b, e);
    if (lo > b) lp_qsort4<D - 1>(p, v, b, lo - 1);
    if (lo < e) lp_qsort4<D - 1>(p, v, lo + 1, e);
  }
}
// get_permutation_index (liop.c:250-262)
MX_D int lp_perm_index(unsigned p) {
  int q[4] = {(int)lp_get(p, 0), (int)lp_get(p, 1), (int)lp_get(p, 2), (int)lp_get(p, 3)};
  int index = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    index = index * (4 - i) + q[i];
#pragma unroll
    for (int j = i + 1; j < 4; j++) if (q[j] > q[i]) q[j]--;
  }
  return index;
}

// patches: [n][1681] f32 (rows 4-byte aligned); out: [*][144] f32, row jobs[k].outIdx (jobs != nullptr) or k.
// dbgPath / dbgPerm (optional): [n] path taken (0 fast, 1 exact) and [n][673] the permutation the bins were cut from.
__global__ __launch_bounds__(LP_T) void k_liop(const float *__restrict__ patches, int n, float *__restrict__ out, const DescJob *__restrict__ jobs,
                                               const unsigned short *__restrict__ pixels, const LiopSample *__restrict__ samples,
                                               unsigned *exactCount, int *dbgPath, int *dbgPerm) {
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= n) return;
  __shared__ float spatch[LP_NPX];
  __shared__ unsigned long long skey[LP_SORT];
  __shared__ float sk[LP_N];                 // intensity of measurement pixel i, -0 stored as +0
  __shared__ unsigned short sperm[LP_N];     // measurement pixel of rank r
  __shared__ int shist[LP_DIM];
  __shared__ int sstack[LP_STACK][2];
  __shared__ int sssq;
  const float *src = patches + (size_t)k * LP_NPX;
  for (int i = tid; i < LP_NPX; i += LP_T) spatch[i] = src[i];
  if (tid < LP_DIM) shist[tid] = 0;
  if (tid == 0) sssq = 0;
  __syncthreads();
  for (int i = tid; i < LP_SORT; i += LP_T) {
    unsigned long long key = ~0ull;
    if (i < LP_N) {
      unsigned u = __float_as_uint(spatch[pixels[i]]);
      if (u == 0x80000000u) u = 0;
      sk[i] = __uint_as_float(u);
      u = (u >> 31) ? ~u : (u | 0x80000000u);        // finite floats order like these words
      key = ((unsigned long long)u << 32) | (unsigned)i;
    }
    skey[i] = key;
  }
  __syncthreads();
  for (int kk = 2; kk <= LP_SORT; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < LP_SORT / 2; t += LP_T) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long a = skey[i], b = skey[l];
        if ((a > b) == ((i & kk) == 0)) { skey[i] = b; skey[l] = a; }
      }
      __syncthreads();
    }
  // a group of equal intensities across a cut: ranks 112 e - 1 and 112 e hold the same key
  const bool mine = tid >= 1 && tid < LP_BINS && (unsigned)(skey[LP_AREA * tid - 1] >> 32) == (unsigned)(skey[LP_AREA * tid] >> 32);
  const int exact = __syncthreads_or(mine);
  for (int r = tid; r < LP_N; r += LP_T) sperm[r] = exact ? (unsigned short)r : (unsigned short)skey[r];
  __syncthreads();
  if (exact) {
    if (tid == 0) {
      if (exactCount) atomicAdd(exactCount, 1u);
      // patch_sort on the identity permutation.  A segment [b, e] of the quicksort holds the elements of the sorted ranks b .. e,
      // so its maximum is the sorted key of rank e.  The two sub-segments are independent: the larger is stacked, the smaller
      // is next (at most log2(673) + 1 stacked).
      int sp = 1;
      sstack[0][0] = 0; sstack[0][1] = LP_N - 1;
      while (sp > 0) {
        sp--;
        int b = sstack[sp][0], e = sstack[sp][1];
        while (b < e) {
          const int mid = (b + e) >> 1;
          const unsigned short pv = sperm[mid];
          sperm[mid] = sperm[e]; sperm[e] = pv;
          const float kp = sk[pv];
          if (kp == sk[(unsigned short)skey[e]]) { e--; continue; }    // every element <= pivot: nothing moves, the pivot stays last
          int lo = b;
          for (int i = b; i < e; i++) {
            const unsigned short x = sperm[i];
            if (sk[x] <= kp) { const unsigned short y = sperm[lo]; sperm[lo] = x; sperm[i] = y; lo++; }
          }
          { const unsigned short y = sperm[lo]; sperm[lo] = sperm[e]; sperm[e] = y; }
          const int nl = lo - b, nr = e - lo;
          if (nl <= nr) {
            if (nr > 1 && sp < LP_STACK) { sstack[sp][0] = lo + 1; sstack[sp][1] = e; sp++; }
            e = lo - 1;
          } else {
            if (nl > 1 && sp < LP_STACK) { sstack[sp][0] = b; sstack[sp][1] = lo - 1; sp++; }
            b = lo + 1;
          }
        }
      }
    }
    __syncthreads();
  }
  // threshold = -intensityThreshold * (Imax - Imin), f32 (liop.c:464-471)
  const float thrF = (float)(5.0 / 255) * (sk[sperm[LP_N - 1]] - sk[sperm[0]]);
  const double thr = (double)thrF;
  for (int r = tid; r < LP_N; r += LP_T) {
    const int i = sperm[r];
    const int bin = r / LP_AREA < LP_BINS - 1 ? r / LP_AREA : LP_BINS - 1;
    float v[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const LiopSample S = samples[i * 4 + t];
      const int ix = S.ix, iy = S.iy, o = ix + iy * LP_SIDE;
      // liop.c:513-516 with its bound tests (ix < L, not ix + 1 < L); an operand outside the patch's 1681 floats is 0.0
      const int oa = (ix >= 0 && iy >= 0) ? o : -1, ob = (ix < LP_SIDE && iy >= 0) ? o + 1 : -1;
      const int oc = (ix >= 0 && iy < LP_SIDE) ? o + LP_SIDE : -1, od = (ix < LP_SIDE && iy < LP_SIDE) ? o + LP_SIDE + 1 : -1;
      const double a = (oa >= 0 && oa < LP_NPX) ? (double)spatch[oa] : 0.0, b = (ob >= 0 && ob < LP_NPX) ? (double)spatch[ob] : 0.0;
      const double c = (oc >= 0 && oc < LP_NPX) ? (double)spatch[oc] : 0.0, d = (od >= 0 && od < LP_NPX) ? (double)spatch[od] : 0.0;
      const double wx = S.wx, wy = S.wy;
      v[t] = (float)((1 - wy) * (a + (b - a) * wx) + wy * (c + (d - c) * wx));
    }
    unsigned p = 0x3210u;
    lp_qsort4<3>(p, v, 0, 3);
    const int pidx = lp_perm_index(p);
    int w = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int t = q + 1; t < 4; t++) {
        const double a = (double)v[q], b = (double)v[t];
        w += (a > b + thr || b > a + thr) ? 1 : 0;
      }
    if (w) atomicAdd(&shist[pidx + 24 * bin], w);
  }
  __syncthreads();
  // a bin holds an integer <= 6 * 673 and the squares sum to less than 2^24: every f32 partial sum of liop.c:546-549 is exact
  if (tid < LP_DIM) atomicAdd(&sssq, shist[tid] * shist[tid]);
  __syncthreads();
  if (tid < LP_DIM) {
    const double len = sqrt((double)(float)sssq);
    const float norm = (float)(len > 1e-12 ? len : 1e-12);        // VL_MAX(sqrt(norm), 1e-12), stored to the f32 `norm`
    const size_t row = jobs ? (size_t)jobs[k].outIdx : (size_t)k;
    out[row * LP_DIM + tid] = (float)shist[tid] / norm;
  }
  if (dbgPath && tid == 0) dbgPath[k] = exact ? 1 : 0;
  if (dbgPerm) for (int r = tid; r < LP_N; r += LP_T) dbgPerm[(size_t)k * LP_N + r] = sperm[r];
}

void launch_liop(hipStream_t s, const float *patches, int n, float *out, const DescJob *jobs, const unsigned short *pixels,
                 const LiopSample *samples, unsigned *exactCount, int *dbgPath, int *dbgPerm) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_liop, dim3(n), dim3(LP_T), 0, s, patches, n, out, jobs, pixels, samples, exactCount, dbgPath, dbgPerm);
}

}  // namespace mx
