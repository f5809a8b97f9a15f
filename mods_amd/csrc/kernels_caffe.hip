// kernels_caffe.hip -- the learned-descriptor front end: the network's input blob and the normalisation of its output rows.
//
// Reference: the "CAFFE" branch of SynthDetectDescribeKeypoints, imagerepresentation.cpp:1343-1534
//   interpolate (P x P patch of every plane of OriginalImg, A * curr_sc)      detectors/helpers.cpp:551-626
//   convertTo(CV_8UC3) / convertTo(CV_8U) + GRAY2BGR, CVMatToDatum, - mean_px   imagerepresentation.cpp:1410-1489
//   L2normalize / L1normalize / RootNormalize                                   imagerepresentation.cpp:181-217
// k_caffe_patches: one workgroup per region, one lane per patch row (one to four wavefronts).  A lane runs the f32 running sums
// of interpolate() along its row -- the coordinates are computed once and serve the taps of every plane -- and leaves the bytes
// of CAFFE_COLS columns in an LDS tile; the workgroup then stores the tile as f32, one patch row segment per wavefront and
// instruction, so that the blob (12 P^2 bytes per region against P^2 bytes of LDS traffic per plane) leaves in row stores.
// k_caffe_norm: one lane per row for the sums, the rows of a wavefront move through a [16][128] LDS tile so that global memory is
// read along the rows while every lane walks its own row in order: the f64 sum of a row is one chain, i = 0 .. dim - 1.
#include "engine.hpp"

namespace mx {

constexpr int CAFFE_U = 4;      // samples of a row in flight per lane: 4 taps each on up to three planes

// saturate_cast<uchar>(float): cvRound (to nearest, ties to even), then the clamp to 0 .. 255; NaN gives 0
MX_D unsigned char caffe_u8(float v) {
  const float r = fminf(fmaxf(rintf(v), 0.f), 255.f);
  return (unsigned char)(int)r;
}

template <int NP>
__global__ __launch_bounds__(256) void k_caffe_patches(const CaffeJob *jobs, int n, const float *q0, const float *q1, const float *q2,
                                                       int rows, int cols, int P, CaffeGeo g, float m0, float m1, float m2, float *out,
                                                       unsigned char *flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tile[];   // [NP][P][g.stride] bytes of the chunk's columns
  const int k = xcd_chunk(blockIdx.x, n);   // regions sorted by position share image lines: one part of the list per XCD's L2
  if (k >= n) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwaves = blockDim.x >> 6;
  const CaffeJob jb = jobs[k];
  const gcfloat_p p0 = as_global(q0), p1 = as_global(q1), p2 = as_global(q2);
  const int half = P >> 1;
  const bool touch = jb.touch != 0;
  // lane t owns row t: t steps of the running sum of the row starts (helpers.cpp:563-564, 586-587)
  float rx = jb.x - (float)half * jb.a12, ry = jb.y - (float)half * jb.a22;
  for (int j = 0; j < t && j < P - 1; j++) { rx += jb.a12; ry += jb.a22; }
  float WX = rx - (float)half * jb.a11, WY = ry - (float)half * jb.a21;
  bool outside = false;
  float *const o = out + (size_t)k * 3 * P * P;
  for (int c0 = 0; c0 < P; c0 += g.chunkCols) {
    const int cw = min(g.chunkCols, P - c0);
    if (t < P) {
      unsigned char *const row = tile + t * g.stride;
      for (int u0 = 0; u0 < cw; u0 += CAFFE_U) {
        float v[NP][CAFFE_U];
#pragma unroll
        for (int u = 0; u < CAFFE_U; u++) {
          const bool live = u0 + u < cw;      // the same for every lane
          if (!touch) {
            v[0][u] = live ? bilinear_tap(p0, rows, cols, WX, WY, false) : 0.f;
            if constexpr (NP == 3) {
              v[1][u] = live ? bilinear_tap(p1, rows, cols, WX, WY, false) : 0.f;
              v[2][u] = live ? bilinear_tap(p2, rows, cols, WX, WY, false) : 0.f;
            }
          } else {
            v[0][u] = live ? bilinear_tap_touch_select(p0, rows, cols, WX, WY) : 0.f;
            if constexpr (NP == 3) {
              v[1][u] = live ? bilinear_tap_touch_select(p1, rows, cols, WX, WY) : 0.f;
              v[2][u] = live ? bilinear_tap_touch_select(p2, rows, cols, WX, WY) : 0.f;
            }
            if (live) {       // what interpolate() returns: a sample that took the `else` of helpers.cpp:603
              const int x = (int)floorf(WX), y = (int)floorf(WY);
              outside |= !(WX >= 0 && WY >= 0 && x < cols - 1 && y < rows - 1);
            }
          }
          if (live) { WX += jb.a11; WY += jb.a21; }
        }
#pragma unroll
        for (int u = 0; u < CAFFE_U; u++)
          if (u0 + u < cw) {
#pragma unroll
            for (int c = 0; c < NP; c++) row[c * g.planeBytes + u0 + u] = caffe_u8(v[c][u]);
          }
      }
    }
    __syncthreads();
    // CVMatToDatum's order: channel, row, column.  A wavefront takes one (channel, row) at a time and stores its cw columns
    for (int r = wave; r < 3 * P; r += nwaves) {
      const int c = r >= 2 * P ? 2 : (r >= P ? 1 : 0), h = r - c * P;
      if (lane < cw) {
        const float b = (float)tile[(NP == 3 ? c : 0) * g.planeBytes + h * g.stride + lane];   // GRAY2BGR: the one byte three times
        o[((size_t)c * P + h) * P + c0 + lane] = b - (c == 0 ? m0 : (c == 1 ? m1 : m2));
      }
    }
    __syncthreads();
  }
  const int any = __syncthreads_or(outside ? 1 : 0);
  if (flags && t == 0) flags[k] = (unsigned char)((touch ? 1 : 0) | (any ? 2 : 0));
}

void launch_caffe_patches(hipStream_t s, const CaffeJob *jobs, int n, const float *p0, const float *p1, const float *p2, int nplanes,
                          int rows, int cols, int P, float m0, float m1, float m2, float *out, unsigned char *flags) {
  const CaffeGeo g = caffe_geometry(P);
  const dim3 grid(8 * ((n + 7) / 8)), block(64 * g.waves);
  if (nplanes == 3)
    hipLaunchKernelGGL(k_caffe_patches<3>, grid, block, (size_t)3 * g.planeBytes, s, jobs, n, p0, p1, p2, rows, cols, P, g, m0, m1, m2, out, flags);
  else
    hipLaunchKernelGGL(k_caffe_patches<1>, grid, block, (size_t)g.planeBytes, s, jobs, n, p0, p0, p0, rows, cols, P, g, m0, m1, m2, out, flags);
}

// NORM: MODSX_CAFFE_NORM_L2 / _L1 / _ROOTL2 (a copy needs no kernel).  One wavefront takes CAFFE_NORM_ROWS rows.  The sum: the
// wavefront moves CAFFE_NORM_COLS columns of its rows at a time through LDS (every load instruction reads 64 consecutive floats
// of one row; the next tile is on its way in registers while this one is summed) and lane r walks row r of the tile in order.
// The outputs need no order: every lane finishes the elements it loads, with the row's coefficient from LDS.
template <int NORM>
__global__ __launch_bounds__(64) void k_caffe_norm(const float *rows, int n, int dim, float *out) {
  constexpr int R = CAFFE_NORM_ROWS, TC = CAFFE_NORM_COLS, PER = R * TC / 64;     // PER elements of a tile per lane
  static_assert(TC == 128 && PER == 2 * R, "element i of a lane: row i >> 1, column ((i & 1) << 6) + lane");
  __shared__ float tile[R][TC + 1];
  __shared__ double coefs[R];
  const int lane = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * R;
  const int nr = (int)min((size_t)R, (size_t)n - first);
  const float *const src = rows + first * dim;
  float *const dst = out + first * dim;
  auto load = [&](int c0, float (&v)[PER]) {
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int r = i >> 1, c = c0 + ((i & 1) << 6) + lane;
      v[i] = (r < nr && c < dim) ? src[(size_t)r * dim + c] : 0.f;
    }
  };
  float cur[PER], nxt[PER];
  load(0, cur);
  double norm = 0.0;
  for (int c0 = 0; c0 < dim; c0 += TC) {
#pragma unroll
    for (int i = 0; i < PER; i++) tile[i >> 1][((i & 1) << 6) + lane] = cur[i];
    __syncthreads();
    if (c0 + TC < dim) load(c0 + TC, nxt);
    if (lane < nr) {
      const int cw = min(TC, dim - c0);
      for (int j = 0; j < cw; j++) {
        const float x = tile[lane][j];
        if (NORM == MODSX_CAFFE_NORM_L2) norm += (double)(x * x);     // the f32 product, widened (imagerepresentation.cpp:185)
        else norm += (double)x;                                        // the signed sum (:197, :210)
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; i++) cur[i] = nxt[i];
  }
  if (lane < nr) coefs[lane] = NORM == MODSX_CAFFE_NORM_L2 ? 1.0 / sqrt(norm) : 1.0 / norm;
  __syncthreads();
  // out may be rows: an element is read and written by the same lane, and the tile loaded ahead lies in other columns
  load(0, cur);
  for (int c0 = 0; c0 < dim; c0 += TC) {
    if (c0 + TC < dim) load(c0 + TC, nxt);
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int r = i >> 1, c = c0 + ((i & 1) << 6) + lane;
      if (r < nr && c < dim) {
        const double v = 512.0 * coefs[r] * (double)cur[i];
        dst[(size_t)r * dim + c] = NORM == MODSX_CAFFE_NORM_ROOTL2 ? (float)sqrt(v) : (float)floor(v);
      }
    }
#pragma unroll
    for (int i = 0; i < PER; i++) cur[i] = nxt[i];
  }
}

void launch_caffe_norm(hipStream_t s, const float *rows, int n, int dim, int norm, float *out) {
  const dim3 grid((n + CAFFE_NORM_ROWS - 1) / CAFFE_NORM_ROWS), block(64);
  if (norm == MODSX_CAFFE_NORM_L2) hipLaunchKernelGGL(k_caffe_norm<MODSX_CAFFE_NORM_L2>, grid, block, 0, s, rows, n, dim, out);
  else if (norm == MODSX_CAFFE_NORM_L1) hipLaunchKernelGGL(k_caffe_norm<MODSX_CAFFE_NORM_L1>, grid, block, 0, s, rows, n, dim, out);
  else hipLaunchKernelGGL(k_caffe_norm<MODSX_CAFFE_NORM_ROOTL2>, grid, block, 0, s, rows, n, dim, out);
}

}  // namespace mx
