// kernels_kaze.hip -- the KAZE detector (AKAZE's nonlinear scale space and Hessian extrema) on whole views.
//
// Reference: the KAZE branch                                      imagerepresentation.cpp:678-681, 1132-1152
//   Create_Nonlinear_Scale_Space, Compute_Multiscale_Derivatives,
//   Compute_Determinant_Hessian_Response, Find_Scale_Space_Extrema  akaze/src/lib/AKAZE.cpp:103-388
//   image_derivatives_scharr, pm_g2, compute_k_percentile,
//   compute_scharr_derivatives, nld_step_scalar, halfsample_image,
//   compute_derivative_kernels                                      akaze/src/lib/nldiffusion_functions.cpp
// The OpenCV calls those sources make (Scharr, sepFilter2D, resize, the Mat expressions) are computed as include/modsx.h states
// them.  Every kernel reads a run of the job table (one KzJob per image and stage) and finds its image through the jobs' first
// workgroups, so a view set is one launch per stage.  Each stage keeps the reference's operations and their order:
//   k_kz_scale    g = p * (float)(1.0 / 255.0).
//   k_kz_first    both first derivatives of a plane at distance s: Lx = columns(smooth) of rows(deriv), Ly = columns(deriv) of
//                 rows(smooth), from an LDS tile with a halo of s (BORDER_REFLECT_101), reading only the three non-zero taps of each
//                 pass (the zero taps add +-0, which nothing downstream tells from 0).  The tile body comes in with 16-byte loads
//                 where the plane allows it.  Four epilogues: store Lx and Ly; store pm_g2 (Scharr's taps 3, 10, 3 at s = 1); the
//                 maximum of the gradient norm over the inner pixels by integer atomic max on the float's bits; its histogram
//                 by integer atomic adds.
//   k_kz_second   Lxx, Lxy, Lyy from tiles of Lx and Ly in the same way, each times (float)(s * s), and Ldet = lxx * lyy - lxy *
//                 lxy (no FMA: -ffp-contract=off).
//   k_kz_fed      one explicit diffusion step: reads Lt and Lflow, writes the new Lt (double-buffered); the four border strips carry
//                 the reference's one-sided formulas, the corners keep Lstep = 0.
//   k_kz_half     resize(INTER_AREA) to half the size: the 2 x 2 mean where both ratios are exactly 2, else the area table, built
//                 per pixel in f64 as the stand-in builds it.
//   k_kz_scan / k_kz_offsets / k_kz_emit   the 3 x 3 maximum scan in (level, raster) order: flags and tile counts, an exclusive
//                 scan of the counts, and a second pass that stores every maximum at tile offset + rank.  No atomic append.
//   k_kz_gather   the nine Ldet values around every survivor of the host's filter passes.
#include "engine.hpp"

namespace mx {

constexpr int KZ_T = 256;
constexpr int KZ_LW = KZ_TW + 2 * KZ_MAX_S, KZ_LH = KZ_TH + 2 * KZ_MAX_S;      // an LDS tile with the largest halo
static_assert(KZ_TW == 64 && KZ_T == 256 && KZ_TH % 4 == 0, "256 threads cover 64 columns x 4 rows per step");
static_assert(KZ_TILE % 64 == 0 && KZ_TILE <= 1024, "a scan tile is a whole number of waves");

// the job of workgroup blk: the last one of the run with blk0 <= blk
MX_D int kz_find(const KzJob *__restrict__ jobs, int n, int blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

MX_D int kz_reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; }
  return p;
}

__global__ __launch_bounds__(KZ_T) void k_kz_scale(const KzJob *__restrict__ jobs, int njobs) {
  const KzJob &J = jobs[kz_find(jobs, njobs, blockIdx.x)];
  const size_t i = (size_t)(blockIdx.x - J.blk0) * KZ_T + threadIdx.x;
  if (i < (size_t)J.rows * J.cols) J.out0[i] = J.in0[i] * (float)(1.0 / 255.0);
}

// tile [KZ_LH][KZ_LW] <- the (KZ_TH + 2 s) x (KZ_TW + 2 s) window of src whose body starts at (y0, x0), BORDER_REFLECT_101
MX_D void kz_load_tile(float (*tile)[KZ_LW], const float *__restrict__ src, int rows, int cols, int y0, int x0, int s) {
  const int th = KZ_TH + 2 * s, tw = KZ_TW + 2 * s;
  const bool vec = (cols & 3) == 0 && x0 + KZ_TW <= cols && (((size_t)src) & 15) == 0;
  if (vec) {      // the body columns in 16-byte loads, then the two halo strips
    for (int i = threadIdx.x; i < th * (KZ_TW / 4); i += KZ_T) {
      const int ly = i / (KZ_TW / 4), q = i - ly * (KZ_TW / 4);
      const int gy = kz_reflect101(y0 - s + ly, rows);
      const float4 v = *(const float4 *)(src + (size_t)gy * cols + x0 + 4 * q);
      float *d = &tile[ly][s + 4 * q];
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    for (int i = threadIdx.x; i < th * 2 * s; i += KZ_T) {
      const int ly = i / (2 * s), h = i - ly * (2 * s);
      const int lx = h < s ? h : KZ_TW + h;
      tile[ly][lx] = src[(size_t)kz_reflect101(y0 - s + ly, rows) * cols + kz_reflect101(x0 - s + lx, cols)];
    }
  } else {
    for (int i = threadIdx.x; i < th * tw; i += KZ_T) {
      const int ly = i / tw, lx = i - ly * tw;
      tile[ly][lx] = src[(size_t)kz_reflect101(y0 - s + ly, rows) * cols + kz_reflect101(x0 - s + lx, cols)];
    }
  }
}

// one pass of sepFilter2D over the three non-zero taps, in ascending index order from the first product
MX_D float kz_deriv(float a, float b) { float v = a * -1.0f; v = v + b * 1.0f; return v; }
MX_D float kz_smooth(float a, float m, float b, float t0, float t1, float t2) { float v = a * t0; v = v + m * t1; v = v + b * t2; return v; }

template <int MODE>
__global__ __launch_bounds__(KZ_T) void k_kz_first(const KzJob *__restrict__ jobs, int njobs, const float *__restrict__ kinv,
                                                   unsigned *__restrict__ hist, int nbins) {
  __shared__ float tile[KZ_LH][KZ_LW];
  __shared__ float rd[KZ_LH][KZ_TW], rs[KZ_LH][KZ_TW];
  __shared__ unsigned wmax;
  const KzJob &J = jobs[kz_find(jobs, njobs, blockIdx.x)];
  const int t = blockIdx.x - J.blk0, ty = t / J.tilesX, tx = t - ty * J.tilesX;
  const int y0 = ty * KZ_TH, x0 = tx * KZ_TW, s = J.s, rows = J.rows, cols = J.cols;
  const float t0 = J.t0, t1 = J.t1, t2 = J.t2;
  if (MODE == KZ_MAX && threadIdx.x == 0) wmax = 0;
  kz_load_tile(tile, J.in0, rows, cols, y0, x0, s);
  __syncthreads();
  for (int i = threadIdx.x; i < (KZ_TH + 2 * s) * KZ_TW; i += KZ_T) {
    const int ly = i / KZ_TW, lx = i - ly * KZ_TW;
    const float a = tile[ly][lx], m = tile[ly][lx + s], b = tile[ly][lx + 2 * s];
    rd[ly][lx] = kz_deriv(a, b);
    rs[ly][lx] = kz_smooth(a, m, b, t0, t1, t2);
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, x = x0 + lx;
  unsigned best = 0;
  for (int ly = threadIdx.x >> 6; ly < KZ_TH; ly += 4) {
    const int y = y0 + ly;
    if (x >= cols || y >= rows) continue;
    const float Lx = kz_smooth(rd[ly][lx], rd[ly + s][lx], rd[ly + 2 * s][lx], t0, t1, t2);
    const float Ly = kz_deriv(rs[ly][lx], rs[ly + 2 * s][lx]);
    const size_t o = (size_t)y * cols + x;
    if (MODE == KZ_DERIV) { J.out0[o] = Lx; J.out1[o] = Ly; }
    if (MODE == KZ_FLOW) {      // pm_g2: 1.0 / (1.0 + (Lx.mul(Lx) + Ly.mul(Ly)) / (k * k))
      float v = Lx * Lx + Ly * Ly;
      v = v * kinv[J.slot * KZ_MAX_OCTAVES + J.octave];
      v = 1.0f + v;
      J.out0[o] = 1.0f / v;
    }
    if (MODE == KZ_MAX || MODE == KZ_HIST) {
      if (y < 1 || y > rows - 2 || x < 1 || x > cols - 2) continue;
      const float modg = sqrtf(Lx * Lx + Ly * Ly);
      if (MODE == KZ_MAX) { if (modg == modg) best = max(best, __float_as_uint(modg)); }
      else if (modg != 0.0f) {
        const float hmax = __uint_as_float(hist[(size_t)J.slot * (nbins + 1)]);
        long long nbin = (long long)floorf((float)nbins * (modg / hmax));
        if (nbin == nbins) nbin--;
        if (nbin >= 0 && nbin < nbins) atomicAdd(&hist[(size_t)J.slot * (nbins + 1) + 1 + nbin], 1u);
      }
    }
  }
  if (MODE == KZ_MAX) {
    atomicMax(&wmax, best);
    __syncthreads();
    if (threadIdx.x == 0 && wmax) atomicMax(&hist[(size_t)J.slot * (nbins + 1)], wmax);
  }
}

__global__ __launch_bounds__(KZ_T) void k_kz_second(const KzJob *__restrict__ jobs, int njobs) {
  __shared__ float tile[KZ_LH][KZ_LW];
  __shared__ float rdx[KZ_LH][KZ_TW], rsx[KZ_LH][KZ_TW], rsy[KZ_LH][KZ_TW];
  const KzJob &J = jobs[kz_find(jobs, njobs, blockIdx.x)];
  const int t = blockIdx.x - J.blk0, ty = t / J.tilesX, tx = t - ty * J.tilesX;
  const int y0 = ty * KZ_TH, x0 = tx * KZ_TW, s = J.s, rows = J.rows, cols = J.cols;
  const float t0 = J.t0, t1 = J.t1, t2 = J.t2;
  kz_load_tile(tile, J.in0, rows, cols, y0, x0, s);      // Lx
  __syncthreads();
  for (int i = threadIdx.x; i < (KZ_TH + 2 * s) * KZ_TW; i += KZ_T) {
    const int ly = i / KZ_TW, lx = i - ly * KZ_TW;
    const float a = tile[ly][lx], m = tile[ly][lx + s], b = tile[ly][lx + 2 * s];
    rdx[ly][lx] = kz_deriv(a, b);
    rsx[ly][lx] = kz_smooth(a, m, b, t0, t1, t2);
  }
  __syncthreads();
  kz_load_tile(tile, J.in1, rows, cols, y0, x0, s);      // Ly
  __syncthreads();
  for (int i = threadIdx.x; i < (KZ_TH + 2 * s) * KZ_TW; i += KZ_T) {
    const int ly = i / KZ_TW, lx = i - ly * KZ_TW;
    rsy[ly][lx] = kz_smooth(tile[ly][lx], tile[ly][lx + s], tile[ly][lx + 2 * s], t0, t1, t2);
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, x = x0 + lx;
  const float ss = J.scale;      // (float)(s * s)
  for (int ly = threadIdx.x >> 6; ly < KZ_TH; ly += 4) {
    const int y = y0 + ly;
    if (x >= cols || y >= rows) continue;
    float lxx = kz_smooth(rdx[ly][lx], rdx[ly + s][lx], rdx[ly + 2 * s][lx], t0, t1, t2);
    float lxy = kz_deriv(rsx[ly][lx], rsx[ly + 2 * s][lx]);
    float lyy = kz_deriv(rsy[ly][lx], rsy[ly + 2 * s][lx]);
    lxx = lxx * ss; lxy = lxy * ss; lyy = lyy * ss;
    J.out0[(size_t)y * cols + x] = (lxx * lyy - lxy * lxy);
  }
}

// nld_step_scalar (nldiffusion_functions.cpp:260-306).  half = 0.5 * stepsize in f64; the sum in brackets is f32
__global__ __launch_bounds__(KZ_T) void k_kz_fed(const KzJob *__restrict__ jobs, int njobs, double half) {
  const KzJob &J = jobs[kz_find(jobs, njobs, blockIdx.x)];
  const int t = blockIdx.x - J.blk0, ty = t / J.tilesX, tx = t - ty * J.tilesX;
  const int rows = J.rows, cols = J.cols;
  const int j = tx * 64 + (threadIdx.x & 63), i = ty * 4 + (threadIdx.x >> 6);
  if (i >= rows || j >= cols) return;
  const float *__restrict__ Ld = J.in0, *__restrict__ c = J.in1;
  const size_t o = (size_t)i * cols + j;
  const bool top = i == 0, bottom = i == rows - 1, left = j == 0, right = j == cols - 1;
  float step = 0.0f;
  if (!((top || bottom) && (left || right))) {
    const float L0 = Ld[o], c0 = c[o];
    float sum;
    if (right) {
      const float xneg = (c[o - 1] + c0) * (L0 - Ld[o - 1]);
      sum = -xneg;
    } else {
      const float xpos = (c0 + c[o + 1]) * (Ld[o + 1] - L0);
      const float xneg = left ? (c0 + c0) * (L0 - L0) : (c[o - 1] + c0) * (L0 - Ld[o - 1]);
      sum = xpos - xneg;
    }
    const float ypos = bottom ? (c0 + c0) * (L0 - L0) : (c0 + c[o + cols]) * (Ld[o + cols] - L0);
    sum = sum + ypos;
    if (!top) {
      const float yneg = (c[o - cols] + c0) * (L0 - Ld[o - cols]);
      sum = sum - yneg;
    }
    step = (float)(half * (double)sum);
  }
  J.out0[o] = Ld[o] + step;
}

// the INTER_AREA table of destination index d of one axis: at most KZ_AREA entries (source index, weight), in table order
constexpr int KZ_AREA = 4;
MX_D int kz_area(int ssize, int dsize, int d, int *si, float *al) {
  const double scale = ssize / (double)dsize;
  const double fs1 = d * scale, fs2 = fs1 + scale, cell = fmin(scale, ssize - fs1);
  int s1 = (int)ceil(fs1), s2 = (int)floor(fs2);
  s2 = min(s2, ssize - 1);
  s1 = min(s1, s2);
  int n = 0;
  if (s1 - fs1 > 1e-3) { si[n] = s1 - 1; al[n] = (float)((s1 - fs1) / cell); n++; }
  for (int s = s1; s < s2 && n < KZ_AREA; s++) { si[n] = s; al[n] = (float)(1.0 / cell); n++; }
  if (fs2 - s2 > 1e-3 && n < KZ_AREA) { si[n] = s2; al[n] = (float)(fmin(fmin(fs2 - s2, 1.), cell) / cell); n++; }
  return n;
}

__global__ __launch_bounds__(KZ_T) void k_kz_half(const KzJob *__restrict__ jobs, int njobs) {
  const KzJob &J = jobs[kz_find(jobs, njobs, blockIdx.x)];
  const int t = blockIdx.x - J.blk0, ty = t / J.tilesX, tx = t - ty * J.tilesX;
  const int rows = J.rows, cols = J.cols, srows = J.srows, scols = J.scols;
  const int x = tx * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
  if (y >= rows || x >= cols) return;
  const float *__restrict__ S = J.in0;
  float v;
  if (srows == 2 * rows && scols == 2 * cols) {
    const float *a = S + (size_t)(2 * y) * scols + 2 * x, *b = a + scols;
    v = (((a[0] + a[1]) + b[0]) + b[1]) * 0.25f;
  } else {
    int xs[KZ_AREA], ys[KZ_AREA];
    float xa[KZ_AREA], ya[KZ_AREA];
    const int nx = kz_area(scols, cols, x, xs, xa), ny = kz_area(srows, rows, y, ys, ya);
    v = 0.0f;
    for (int k = 0; k < ny; k++) {
      const float *row = S + (size_t)ys[k] * scols;
      float buf = 0.0f;
      for (int q = 0; q < nx; q++) buf += row[xs[q]] * xa[q];
      if (k == 0) v = ya[k] * buf; else v += ya[k] * buf;
    }
  }
  J.out0[(size_t)y * cols + x] = v;
}

// the 3 x 3 maximum test of Find_Scale_Space_Extrema (AKAZE.cpp:288-299) at raster position index of the job's Ldet plane
MX_D bool kz_is_max(const KzJob &J, int index, float dthr, float minthr, int &r, int &c, float &value) {
  const int rows = J.rows, cols = J.cols;
  if (index >= rows * cols) return false;
  r = index / cols; c = index - r * cols;
  if (r < 1 || r > rows - 2 || c < 1 || c > cols - 2) return false;
  const float *__restrict__ p = J.in0 + (size_t)r * cols + c;
  value = *p;
  return value > dthr && value >= minthr && value > p[-1] && value > p[1] && value > p[-cols - 1] && value > p[-cols] &&
         value > p[-cols + 1] && value > p[cols - 1] && value > p[cols] && value > p[cols + 1];
}

__global__ __launch_bounds__(KZ_TILE) void k_kz_scan(const KzJob *__restrict__ jobs, int njobs, float dthr, float minthr,
                                                     unsigned char *__restrict__ flags, int *__restrict__ counts) {
  const KzJob &J = jobs[kz_find(jobs, njobs, blockIdx.x)];
  int r, c;
  float v;
  const int flag = kz_is_max(J, (blockIdx.x - J.blk0) * KZ_TILE + threadIdx.x, dthr, minthr, r, c, v) ? 1 : 0;
  flags[(size_t)blockIdx.x * KZ_TILE + threadIdx.x] = (unsigned char)flag;
  const int n = __syncthreads_count(flag);
  if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// offs [n + 1] = the exclusive scan of counts [n]; slotStart [ns + 1] = offs at tile0[s] (tile0[ns] = n).  One workgroup
constexpr int KZ_SCAN_T = 1024;
__global__ __launch_bounds__(KZ_SCAN_T) void k_kz_offsets(const int *__restrict__ counts, int n, int *__restrict__ offs,
                                                          const int *__restrict__ tile0, int ns, int *__restrict__ slotStart) {
  __shared__ int sa[KZ_SCAN_T];
  const int t = threadIdx.x, chunk = (n + KZ_SCAN_T - 1) / KZ_SCAN_T;
  const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
  int a = 0;
  for (int k = lo; k < hi; k++) a += counts[k];
  sa[t] = a;
  __syncthreads();
  for (int d = 1; d < KZ_SCAN_T; d <<= 1) {
    const int va = t >= d ? sa[t - d] : 0;
    __syncthreads();
    sa[t] += va;
    __syncthreads();
  }
  int ra = sa[t] - a;
  for (int k = lo; k < hi; k++) { offs[k] = ra; ra += counts[k]; }
  if (t == KZ_SCAN_T - 1) offs[n] = sa[t];
  __syncthreads();
  for (int j = t; j <= ns; j += KZ_SCAN_T) slotStart[j] = offs[tile0[j]];
}

__global__ __launch_bounds__(KZ_TILE) void k_kz_emit(const KzJob *__restrict__ jobs, int njobs, const unsigned char *__restrict__ flags,
                                                     const int *__restrict__ offs, KzRaw *__restrict__ raw, int cap) {
  __shared__ int wn[KZ_TILE / 64];
  const int flag = flags[(size_t)blockIdx.x * KZ_TILE + threadIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag), below = (1ull << lane) - 1;
  if (lane == 0) wn[wave] = __popcll(b);
  __syncthreads();
  if (!flag) return;
  int at = offs[blockIdx.x] + __popcll(b & below);
  for (int w = 0; w < wave; w++) at += wn[w];
  if (at >= cap) return;
  const KzJob &J = jobs[kz_find(jobs, njobs, blockIdx.x)];
  const int index = (blockIdx.x - J.blk0) * KZ_TILE + threadIdx.x;
  KzRaw e;
  e.slot = J.slot; e.level = J.level; e.r = index / J.cols; e.c = index - e.r * J.cols;
  e.value = J.in0[index];
  raw[at] = e;
}

// out [n][9] = the 3 x 3 Ldet values around (y, x) of every item, rows top to bottom
__global__ __launch_bounds__(KZ_T) void k_kz_gather(const KzItem *__restrict__ items, int n, const float *__restrict__ ldet,
                                                    float *__restrict__ out) {
  const int i = blockIdx.x * KZ_T + threadIdx.x;
  if (i >= n) return;
  const KzItem it = items[i];
  const float *__restrict__ p = ldet + it.ofs + (size_t)it.y * it.cols + it.x;
#pragma unroll
  for (int dr = -1; dr <= 1; dr++)
#pragma unroll
    for (int dc = -1; dc <= 1; dc++) out[(size_t)i * 9 + (dr + 1) * 3 + (dc + 1)] = p[dr * it.cols + dc];
}

void launch_kaze_scale(hipStream_t s, const KzJob *jobs, int njobs, int blocks) {
  if (blocks > 0) hipLaunchKernelGGL(k_kz_scale, dim3(blocks), dim3(KZ_T), 0, s, jobs, njobs);
}
void launch_kaze_first(hipStream_t s, int mode, const KzJob *jobs, int njobs, int blocks, const float *kinv, unsigned *hist, int nbins) {
  if (blocks <= 0) return;
  if (mode == KZ_DERIV) hipLaunchKernelGGL(k_kz_first<KZ_DERIV>, dim3(blocks), dim3(KZ_T), 0, s, jobs, njobs, kinv, hist, nbins);
  else if (mode == KZ_FLOW) hipLaunchKernelGGL(k_kz_first<KZ_FLOW>, dim3(blocks), dim3(KZ_T), 0, s, jobs, njobs, kinv, hist, nbins);
  else if (mode == KZ_MAX) hipLaunchKernelGGL(k_kz_first<KZ_MAX>, dim3(blocks), dim3(KZ_T), 0, s, jobs, njobs, kinv, hist, nbins);
  else hipLaunchKernelGGL(k_kz_first<KZ_HIST>, dim3(blocks), dim3(KZ_T), 0, s, jobs, njobs, kinv, hist, nbins);
}
void launch_kaze_second(hipStream_t s, const KzJob *jobs, int njobs, int blocks) {
  if (blocks > 0) hipLaunchKernelGGL(k_kz_second, dim3(blocks), dim3(KZ_T), 0, s, jobs, njobs);
}
void launch_kaze_fed(hipStream_t s, const KzJob *jobs, int njobs, int blocks, float tau) {
  if (blocks > 0) hipLaunchKernelGGL(k_kz_fed, dim3(blocks), dim3(KZ_T), 0, s, jobs, njobs, 0.5 * tau);
}
void launch_kaze_half(hipStream_t s, const KzJob *jobs, int njobs, int blocks) {
  if (blocks > 0) hipLaunchKernelGGL(k_kz_half, dim3(blocks), dim3(KZ_T), 0, s, jobs, njobs);
}
void launch_kaze_scan(hipStream_t s, const KzJob *jobs, int njobs, int tiles, float dthr, float minthr, unsigned char *flags, int *counts,
                      int *offs, const int *tile0, int nslots, int *slotStart) {
  if (tiles > 0) hipLaunchKernelGGL(k_kz_scan, dim3(tiles), dim3(KZ_TILE), 0, s, jobs, njobs, dthr, minthr, flags, counts);
  hipLaunchKernelGGL(k_kz_offsets, dim3(1), dim3(KZ_SCAN_T), 0, s, counts, tiles, offs, tile0, nslots, slotStart);
}
void launch_kaze_emit(hipStream_t s, const KzJob *jobs, int njobs, int tiles, const unsigned char *flags, const int *offs, KzRaw *raw, int cap) {
  if (tiles > 0) hipLaunchKernelGGL(k_kz_emit, dim3(tiles), dim3(KZ_TILE), 0, s, jobs, njobs, flags, offs, raw, cap);
}
void launch_kaze_gather(hipStream_t s, const KzItem *items, int n, const float *ldet, float *out) {
  if (n > 0) hipLaunchKernelGGL(k_kz_gather, dim3((n + KZ_T - 1) / KZ_T), dim3(KZ_T), 0, s, items, n, ldet, out);
}

}  // namespace mx
