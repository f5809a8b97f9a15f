// kernels_surf.hip -- the SURF descriptor functor on a normalised 41 x 41 patch (OpenSURF's upright SURF-64 of one fixed point).
//
// Reference: SURFDescriptor::operator()      descriptors/surfdescriptor.hpp:13-37
//   Integral / getGray                        opensurf/integral.cpp:18-55, opensurf/utils.cpp:62-82
//   Surf::getDescriptor(true), haarX, haarY   opensurf/surf.cpp:152-283
//   BoxIntegral                               opensurf/integral.h:35-53
// The point, its scale and with them every sample coordinate and every gaussian weight are constants of (patchSize, mrSize): the
// host builds them with the reference's expressions and libm's expf (engine_surf.hip: surf_tables), the kernel reads them.
// One wavefront per patch, one patch per workgroup: no wavefront waits for another, and a barrier of a one-wave workgroup costs
// no more than the LDS wait it implies.  Stages, each in the reference's operation order (the order of f32 adds is the result):
//   1. g = p * (float)(1.0 / 255.0) + 0.0f into LDS (cvConvertScale on f32, restated);
//   2. lanes 0 .. 40 run the serial row sums rs of one row each (stride 41 words: no bank conflict);
//   3. lanes 0 .. 40 run one column each: I[r][c] = rs[r][c] + I[r - 1][c];
//   4. the 24 x 24 distinct (k, l) sample positions, lane-parallel: haarX and haarY, four BoxIntegrals of four LDS reads;
//   5. lane 4 q + c runs chain c (dx, dy, mdx, mdy) of sub-region q: 81 ordered adds; the 16 lanes that read the same response
//      share an address (a broadcast), the 16 addresses of a step fall on 16 different banks;
//   6. every lane sums the 16 length terms in order (LDS broadcasts), takes the f32 root and the f64 reciprocal, and stores its
//      entry (float)((double)desc * inv_len): a row of NaN where the length is 0, as the reference gives.
// No sample is skipped: a window beyond the far border does not sum to 0 (r1 == r2 gives (A - B) - A + B, a rounding residue
// that the reference keeps where it is positive), and the windows that are provably empty cost four predicated reads.
#include "engine.hpp"

namespace mx {

constexpr int SF_SIDE = 41, SF_NPX = SF_SIDE * SF_SIDE, SF_NK = 24, SF_NR = SF_NK * SF_NK, SF_DIM = MODSX_SURF_DIM, SF_T = 64;
static_assert(SF_DIM == 64 && SF_T == SF_DIM, "one lane per descriptor entry");

// BoxIntegral (integral.h:35-53): std::max(0.f, v) is v only where 0.f < v
MX_D float sf_box(const float *I, int row, int col, int rows, int cols) {
  const int r1 = min(row, SF_SIDE) - 1, c1 = min(col, SF_SIDE) - 1, r2 = min(row + rows, SF_SIDE) - 1, c2 = min(col + cols, SF_SIDE) - 1;
  float A = 0.0f, B = 0.0f, C = 0.0f, D = 0.0f;
  if (r1 >= 0 && c1 >= 0) A = I[r1 * SF_SIDE + c1];
  if (r1 >= 0 && c2 >= 0) B = I[r1 * SF_SIDE + c2];
  if (r2 >= 0 && c1 >= 0) C = I[r2 * SF_SIDE + c1];
  if (r2 >= 0 && c2 >= 0) D = I[r2 * SF_SIDE + c2];
  const float v = A - B - C + D;
  return 0.f < v ? v : 0.f;
}

// patches: [n][1681] f32 (rows 4-byte aligned); out: [*][64] f32, row jobs[k].outIdx (jobs != nullptr) or k
__global__ __launch_bounds__(SF_T) void k_surf(const float *__restrict__ patches, int n, float *__restrict__ out,
                                               const DescJob *__restrict__ jobs, const SurfTab *__restrict__ tab) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  __shared__ float sI[SF_NPX];
  __shared__ float srx[SF_NR], sry[SF_NR];
  __shared__ float slen[16];
  const float *src = patches + (size_t)k * SF_NPX;
  const float gscale = (float)(1.0 / 255.0), gshift = 0.0f;
  for (int i = lane; i < SF_NPX; i += SF_T) sI[i] = src[i] * gscale + gshift;
  __syncthreads();
  if (lane < SF_SIDE) {
    float rs = 0.0f;
    for (int c = 0; c < SF_SIDE; c++) { rs += sI[lane * SF_SIDE + c]; sI[lane * SF_SIDE + c] = rs; }
  }
  __syncthreads();
  if (lane < SF_SIDE) {
    float above = sI[lane];
    for (int r = 1; r < SF_SIDE; r++) { above = sI[r * SF_SIDE + lane] + above; sI[r * SF_SIDE + lane] = above; }
  }
  __syncthreads();
  const int s = tab->haar, h = s / 2;
  for (int p = lane; p < SF_NR; p += SF_T) {
    const int column = tab->sx[p / SF_NK], row = tab->sy[p % SF_NK];
    srx[p] = sf_box(sI, row - h, column, s, h) - 1 * sf_box(sI, row - h, column - h, s, h);
    sry[p] = sf_box(sI, row, column - h, h, s) - 1 * sf_box(sI, row - h, column - h, h, s);
  }
  __syncthreads();
  const int q = lane >> 2, c = lane & 3, k0 = 5 * (q >> 2), l0 = 5 * (q & 3);
  const float co = 1.0f, si = 0.0f;
  const float *w1 = tab->w1 + q * 81;
  float acc = 0.f;
  for (int kk = 0, t = 0; kk < 9; kk++)
    for (int ll = 0; ll < 9; ll++, t++) {
      const int p = (k0 + kk) * SF_NK + l0 + ll;
      const float gauss_s1 = w1[t], rx = srx[p], ry = sry[p];
      const float rrx = gauss_s1 * (-rx * si + ry * co), rry = gauss_s1 * (rx * co + ry * si);
      acc += c == 0 ? rrx : (c == 1 ? rry : (c == 2 ? fabsf(rrx) : fabsf(rry)));
    }
  const float gauss_s2 = tab->w2[q];
  const float dx = __shfl(acc, 4 * q), dy = __shfl(acc, 4 * q + 1), mdx = __shfl(acc, 4 * q + 2), mdy = __shfl(acc, 4 * q + 3);
  if (c == 0) slen[q] = (dx * dx + dy * dy + mdx * mdx + mdy * mdy) * gauss_s2 * gauss_s2;
  __syncthreads();
  float len = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) len += slen[i];
  len = sqrtf(len);
  const double inv_len = 1.0 / (double)len;
  const size_t orow = jobs ? (size_t)jobs[k].outIdx : (size_t)k;
  out[orow * SF_DIM + lane] = (float)((double)(acc * gauss_s2) * inv_len);
}

void launch_surf(hipStream_t s, const float *patches, int n, float *out, const DescJob *jobs, const SurfTab *tab) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_surf, dim3(n), dim3(SF_T), 0, s, patches, n, out, jobs, tab);
}

}  // namespace mx
