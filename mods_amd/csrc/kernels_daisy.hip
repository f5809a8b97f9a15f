// kernels_daisy.hip -- the DAISY descriptor functor on a normalised 41 x 41 patch (libdaisy's descriptor of one fixed point).
//
// Reference: DAISYDescriptor::operator()                      descriptors/daisydescriptor.hpp:51-80
//   set_image, get_descriptor, bi_get_histogram                libdaisy/include/daisy/daisy.h:78-89, 450-503, 536-584
//   initialize, smooth_layers, compute_smoothed_gradient_layers, normalize_*   libdaisy/src/daisy.cpp
//   layered_gradient, gradient, l2norm, divide                 libdaisy/include/kutility/math.hpp
//   conv_horizontal, conv_vertical, conv_buffer_               libdaisy/include/kutility/convolution_default.h
// Everything that is a constant of (rad, radq, thq) -- filter taps, (kos, zin) of the layers, the cube, pixel and bilinear
// weights of every grid point -- is built by the host with the reference's expressions (engine_daisy.hip: daisy_tables).
//
// One workgroup of 8 wavefronts per patch; the whole chain of a patch lives in LDS (18 planes of 41 x 41 f32 = 121 KB):
//   1. all waves: bytes (rint, saturated) * (float)(1.0 / 255.0), the 5-tap blur over rows, then over columns, dx and dy.  The
//      three scratch planes of this stage are planes of waves 0 and 1, which are free until stage 2;
//   2. wave l owns layer l = max(kos_l dx + zin_l dy, 0) in its two planes A, B and filters it 1 + radq times, rows A -> B, then
//      columns B -> A: out[i] = the chain sum = 0; sum += in[clamp(i + j - ksize / 2)] * k[j], j = 0 .. ksize - 1, mul and add
//      unfused (-ffp-contract=off), which is conv_buffer_ on a buffer with replicated borders;
//   3. after the column pass that completes cube c, lanes g < npts of wave l whose grid point selects cube c and is sampled write
//      row[8 g + l] = w0 A + w1 C + w2 B + w3 D, left to right; skipped and zeroed points keep the 0 the row starts with;
//   4. normalisation by the first `dim` threads, each holding one entry; the norms are ordered f32 sums that every thread forms
//      redundantly from LDS broadcasts; the NRM_SIFT rounds run here.
// A pass gives each lane 7 consecutive outputs along the filtered axis (41 lines x 6 segments = 246 work items per plane): a
// sample is read from LDS once and feeds the 7 chains it belongs to, each chain still in its own tap order, so a pass reads
// about ksize + 6 words per 7 outputs instead of 7 ksize (dz_pass: how the ends of the window are handled).  Lanes run along
// the other axis: in the row pass consecutive lanes are 41 words apart (41 is odd: 32 consecutive lines fall on 32 banks), in
// the column pass 1 word apart.  The taps are uniform and come through scalar loads.  After the byte conversion every value is
// finite and at most 1, so no stage can produce an infinity.
#include "engine.hpp"

namespace mx {

constexpr int DZ_SIDE = 41, DZ_NPX = DZ_SIDE * DZ_SIDE, DZ_WAVES = 8, DZ_T = 64 * DZ_WAVES, DZ_SEG = 7, DZ_NSEG = 6;
constexpr int DZ_ITEMS = DZ_SIDE * DZ_NSEG, DZ_PLANES = 2 + 2 * DZ_WAVES, DZ_BLK = 8;
static_assert(DAISY_TAP_PAD == DZ_SEG - 1, "output r of an item is DZ_SEG - 1 - r entries into the padded tap row");
static_assert(DZ_SEG * DZ_NSEG >= DZ_SIDE && DZ_WAVES == 8, "6 segments of 7 cover a line; one wave per layer");
static_assert((DZ_PLANES * DZ_NPX + MODSX_DAISY_MAX_DIM) * 4 <= 160 * 1024, "a patch fits the LDS of a CU");

// one filter pass of a plane by one wavefront: ROWS filters along a row (conv_horizontal), else along a column (conv_vertical)
// taps: a row of the table, DAISY_TAP_PAD zeros in front of the ks taps and zeros behind them (engine.hpp: DaisyTab).  Sample j of
// an item's window feeds output o0 + r with tap j - r, which is entry j - r + 6 of the padded row; a tap outside 0 .. ks - 1 is
// a zero of the padding.  Such a step adds v * 0 = +-0 to a chain, which leaves it as it is: v is finite, and a chain is never
// -0 (it starts at +0, +0 + -0 is +0 and x + -x is +0 under round to nearest).  So every step is the same code, in blocks of 8
// samples: 8 LDS reads and a window of 14 uniform taps in flight, then 56 multiply-adds with constant register indices.
template <bool ROWS>
MX_D void dz_pass(const float *src, float *dst, const float *__restrict__ taps, int ks, int lane) {
  const int half = ks >> 1, nblk = (ks + DZ_SEG - 1 + DZ_BLK - 1) / DZ_BLK;
  for (int u = lane; u < DZ_ITEMS; u += 64) {
    const int a = u % DZ_SIDE, o0 = (u / DZ_SIDE) * DZ_SEG;
    float acc[DZ_SEG];
#pragma unroll
    for (int r = 0; r < DZ_SEG; r++) acc[r] = 0.0f;
    for (int b = 0; b < nblk; b++) {
      const int j = b * DZ_BLK;
      float v[DZ_BLK], t[DZ_BLK + DZ_SEG - 1];
#pragma unroll
      for (int i = 0; i < DZ_BLK; i++) {
        const int q = min(max(o0 + j + i - half, 0), DZ_SIDE - 1);
        v[i] = ROWS ? src[a * DZ_SIDE + q] : src[q * DZ_SIDE + a];
      }
#pragma unroll
      for (int m = 0; m < DZ_BLK + DZ_SEG - 1; m++) t[m] = taps[j + m];
#pragma unroll
      for (int i = 0; i < DZ_BLK; i++)
#pragma unroll
        for (int r = 0; r < DZ_SEG; r++) acc[r] += v[i] * t[i + DZ_SEG - 1 - r];
    }
#pragma unroll
    for (int r = 0; r < DZ_SEG; r++)
      if (o0 + r < DZ_SIDE) dst[ROWS ? a * DZ_SIDE + o0 + r : (o0 + r) * DZ_SIDE + a] = acc[r];
  }
}

// kutility::l2norm of n entries of an LDS row: every lane forms the same ordered sum
MX_D float dz_l2norm(const float *v, int n) {
  float norm = 0.0f;
  for (int k = 0; k < n; k++) norm += v[k] * v[k];
  return sqrtf(norm);
}

// patches: [n][1681] f32 (rows 4-byte aligned); out: [*][tab->dim] f32, row jobs[k].outIdx (jobs != nullptr) or k
__global__ __launch_bounds__(DZ_T) void k_daisy(const float *__restrict__ patches, int n, float *__restrict__ out,
                                                const DescJob *__restrict__ jobs, const DaisyTab *__restrict__ tab, int nrmType) {
  const int k = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (k >= n) return;
  __shared__ float sP[DZ_PLANES * DZ_NPX];
  __shared__ float srow[MODSX_DAISY_MAX_DIM];
  float *sdx = sP, *sdy = sP + DZ_NPX, *A = sP + (2 + 2 * wave) * DZ_NPX, *B = A + DZ_NPX;
  float *s0 = sP + 2 * DZ_NPX, *s1 = s0 + DZ_NPX, *s2 = s1 + DZ_NPX;
  const int dim = tab->dim, npts = tab->npts, nfilt = tab->nfilt;

  // 1. bytes / 255, 5-tap blur, gradient
  const float *src = patches + (size_t)k * DZ_NPX;
  const float inv255 = (float)(1.0 / 255.0);
  for (int i = t; i < DZ_NPX; i += DZ_T) s0[i] = fminf(fmaxf(rintf(src[i]), 0.0f), 255.0f) * inv255;
  if (t < MODSX_DAISY_MAX_DIM) srow[t] = 0.0f;
  __syncthreads();
  for (int i = t; i < DZ_NPX; i += DZ_T) {
    const int r = i / DZ_SIDE, c = i - r * DZ_SIDE;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; j++) sum += s0[r * DZ_SIDE + min(max(c + j - 2, 0), DZ_SIDE - 1)] * tab->k5[j];
    s1[i] = sum;
  }
  __syncthreads();
  for (int i = t; i < DZ_NPX; i += DZ_T) {
    const int r = i / DZ_SIDE, c = i - r * DZ_SIDE;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; j++) sum += s1[min(max(r + j - 2, 0), DZ_SIDE - 1) * DZ_SIDE + c] * tab->k5[j];
    s2[i] = sum;
  }
  __syncthreads();
  for (int i = t; i < DZ_NPX; i += DZ_T) {
    const int r = i / DZ_SIDE, c = i - r * DZ_SIDE;
    // kutility::gradient: the halving is done in double and cast back
    float gx, gy;
    if (c == 0) gx = s2[i + 1] - s2[i];
    else if (c == DZ_SIDE - 1) gx = s2[i] - s2[i - 1];
    else gx = (float)((double)(s2[i + 1] - s2[i - 1]) / 2.0);
    if (r == 0) gy = s2[i + DZ_SIDE] - s2[i];
    else if (r == DZ_SIDE - 1) gy = s2[i] - s2[i - DZ_SIDE];
    else gy = (float)((double)(s2[i + DZ_SIDE] - s2[i - DZ_SIDE]) / 2.0);
    sdx[i] = gx;
    sdy[i] = gy;
  }
  __syncthreads();

  // 2. layer `wave`, then its filters; 3. the grid points of every finished cube.  All waves run the same trip counts, so the
  // workgroup barriers are uniform
  const float kos = tab->kos[wave], zin = tab->zin[wave];
  for (int i = lane; i < DZ_NPX; i += 64) {
    const float value = kos * sdx[i] + zin * sdy[i];
    A[i] = value > 0.0f ? value : 0.0f;
  }
  __syncthreads();
  for (int f = 0; f < nfilt; f++) {
    const float *taps = tab->taps + f * DAISY_TAP_ROW;
    const int ks = tab->fsz[f];
    dz_pass<true>(A, B, taps, ks, lane);
    __syncthreads();
    dz_pass<false>(B, A, taps, ks, lane);
    __syncthreads();
    if (f >= 1 && lane < npts && tab->cube[lane] == f - 1 && tab->state[lane] == 2) {
      const float *p = A + tab->base[lane];
      const float *w = tab->w + 4 * lane;
      float h = w[0] * p[0];
      h += w[1] * p[1];
      h += w[2] * p[DZ_SIDE];
      h += w[3] * p[DZ_SIDE + 1];
      srow[lane * 8 + wave] = h;
    }
  }
  __syncthreads();

  // 4. normalisation
  const bool mine = t < dim;
  float v = mine ? srow[t] : 0.0f;
  if (nrmType == 0) {
    const float norm = dz_l2norm(srow + (mine ? (t & ~7) : 0), 8);
    if (norm != 0.0f) v = v * (float)(1.0 / (double)norm);
  } else if (nrmType == 1) {
    const float norm = dz_l2norm(srow, dim);
    if (norm != 0.0f) v = v * (float)(1.0 / (double)norm);
  } else {
    const float clip = (float)0.154;
    for (int iter = 0; iter < 5; iter++) {
      const float norm = dz_l2norm(srow, dim);
      __syncthreads();
      if ((double)norm > 1e-5) v = v * (float)(1.0 / (double)norm);
      const int clipped = mine && v > clip;
      if (clipped) v = clip;
      if (mine) srow[t] = v;
      if (!__syncthreads_or(clipped)) break;
    }
  }
  if (mine) {
    const size_t orow = jobs ? (size_t)jobs[k].outIdx : (size_t)k;
    out[orow * dim + t] = v;
  }
}

void launch_daisy(hipStream_t s, const float *patches, int n, float *out, const DescJob *jobs, const DaisyTab *tab, int nrmType) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_daisy, dim3(n), dim3(DZ_T), 0, s, patches, n, out, jobs, tab, nrmType);
}

}  // namespace mx
