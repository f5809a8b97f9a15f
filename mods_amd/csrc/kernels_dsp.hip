// kernels_dsp.hip -- the f32 SIFT norm that closes DSP-SIFT (domain-size pooling, imagerepresentation.cpp:1547-1598).
//
// Reference: SIFTDescriptor::SIFTnorm(std::vector<float>&)    matching/siftdesc.cpp:263-278
//            SIFTDescriptor::normalize(std::vector<float>&)   matching/siftdesc.cpp:160-185
// The pooled histogram is a std::vector<float>, so the reference takes the f32 overloads -- not the f64 norm k_describe restates:
// squares, group sums and the length are f32, the factor is 1.0 / (double)len rounded to f32 before the multiply, the clip
// compares in f64, the quantisation multiplies by 512.0f in f32 and adds 0.5 in f64.
//
// A row is 128 values; a half-wave of 32 lanes takes one row, lane q owning bins 4q .. 4q + 3 (the reference's unrolled group
// ((sq0 + sq1) + sq2) + sq3), so a wavefront takes two rows.  The 32 group sums are then added in index order, starting from
// 0.0f, as the reference's serial loop does: every lane of the half-wave runs that chain on values read across lanes, which
// costs what one lane running it would cost and leaves the length in every lane.  Rows are loaded and stored as scalars: the
// device forms promise 4-byte alignment only.  In place is fine: a lane reads its four values before it writes them and no lane
// reads another's.
// Rows are finite.  A row of zeros gives len = 0, fac = inf and NaN values, for which no compare is true; the reference's
// (int) of a NaN is INT_MIN on x86-64 and the clamp makes it 0, so such a row comes out as zeros here too.  NaN and infinities in
// a row give unspecified values and no fault.
#include "engine.hpp"

namespace mx {

constexpr int SN_T = 256, SN_ROWS = SN_T / 32;   // rows per workgroup

__global__ __launch_bounds__(SN_T) void k_sift_norm_f32(const float *rows, int n, double maxBin, float *out) {
  const int lane = threadIdx.x & 31;
  const int row = blockIdx.x * SN_ROWS + (threadIdx.x >> 5);
  const bool alive = row < n;                     // a row past the end repeats the last one and stores nothing
  const size_t base = (size_t)(alive ? row : n - 1) * 128 + 4 * lane;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = rows[base + j];
  const float clipTo = (float)maxBin;
  bool active = true;
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    const float sq0 = v[0] * v[0], sq1 = v[1] * v[1], sq2 = v[2] * v[2], sq3 = v[3] * v[3];
    const float g = sq0 + sq1 + sq2 + sq3;
    float len = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; i++) len += __shfl(g, i, 32);
    len = sqrtf(len);
    const double fac = 1.0 / (double)len;
    const float f = (float)fac;
    bool changed = false;
    if (active) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        v[j] *= f;
        if (pass == 0 && (double)v[j] > maxBin) { v[j] = clipTo; changed = true; }
      }
    }
    // `changed` of the row: the lanes of the other half-wave vote in their own half of the mask
    const unsigned long long any = __ballot(changed);
    const unsigned half = (threadIdx.x & 32) ? (unsigned)(any >> 32) : (unsigned)any;
    if (!half) active = false;                    // the reference leaves after the first pass when nothing was clipped
  }
  if (alive) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const double t = (double)(512.0f * v[j]) + 0.5;
      int b = t == t ? (int)t : 0;
      b = b < 255 ? b : 255;
      b = b > 0 ? b : 0;
      out[base + j] = (float)b;
    }
  }
}

void launch_sift_norm_f32(hipStream_t s, const float *rows, int n, double maxBin, float *out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sift_norm_f32, dim3((n + SN_ROWS - 1) / SN_ROWS), dim3(SN_T), 0, s, rows, n, maxBin, out);
}

}  // namespace mx
