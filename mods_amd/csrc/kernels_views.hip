// kernels_views.hip -- view synthesis on device.
//
// Reference: GenerateSynthImageCorr, synth-detection.cpp:236-430: rotate (cv::warpAffine, INTER_LINEAR,
// BORDER_CONSTANT 128), anisotropic anti-alias blur (cv::GaussianBlur, default BORDER_REFLECT_101), tilt/zoom
// scale (cv::warpAffine again).  The OpenCV 2.4.9 arithmetic restated: inverse map in f64, source coordinates
// in 1/1024 fixed point (cvRound = round half to even), rounded to 1/32 px, weights = products of multiples
// of 1/32 (exact in f32), four taps accumulated left to right in f32.
#include "engine.hpp"

namespace mx {

// cv::warpAffine's fixed-point inverse map: adelta / bdelta depend on x only, X0 / Y0 on y only (OpenCV tabulates the
// former per column and forms the latter per row)
MX_D void warp_xterm(const double *M, int x, int &adelta, int &bdelta) {
  const int AB_SCALE = 1024;
  adelta = (int)rint(M[0] * x * AB_SCALE); bdelta = (int)rint(M[3] * x * AB_SCALE);
}
MX_D void warp_yterm(const double *M, int y, int &X0, int &Y0) {
  const int AB_SCALE = 1024;
  X0 = (int)rint((M[1] * y + M[2]) * AB_SCALE) + 16;
  Y0 = (int)rint((M[4] * y + M[5]) * AB_SCALE) + 16;
}
MX_D float warp_fetch(const float *src, int sh, int sw, float cval, int adelta, int bdelta, int X0, int Y0) {
  const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
  int sx = X >> 5, sy = Y >> 5;
  sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
  sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
  const float fx = (float)(X & 31) * (1.f / 32), fy = (float)(Y & 31) * (1.f / 32);
  const float w0 = (1.f - fy) * (1.f - fx), w1 = (1.f - fy) * fx, w2 = fy * (1.f - fx), w3 = fy * fx;
  float out;
  if (sx >= 0 && sx < sw - 1 && sy >= 0 && sy < sh - 1) {
    // the two taps of a row as ONE 8-byte load (4-byte aligned): the gathers of the rotation are bound by load instructions
    const float *S = src + (size_t)sy * sw + sx;
    float2 a, b;
    __builtin_memcpy(&a, S, 8);
    __builtin_memcpy(&b, S + sw, 8);
    out = a.x * w0 + a.y * w1 + b.x * w2 + b.y * w3;
  } else if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
    out = cval;
  } else {
    const bool x0 = sx >= 0 && sx < sw, x1 = sx + 1 >= 0 && sx + 1 < sw, y0 = sy >= 0 && sy < sh, y1 = sy + 1 >= 0 && sy + 1 < sh;
    const float v0 = (x0 && y0) ? src[(size_t)sy * sw + sx] : cval;
    const float v1 = (x1 && y0) ? src[(size_t)sy * sw + sx + 1] : cval;
    const float v2 = (x0 && y1) ? src[(size_t)(sy + 1) * sw + sx] : cval;
    const float v3 = (x1 && y1) ? src[(size_t)(sy + 1) * sw + sx + 1] : cval;
    out = v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3;
  }
  return out;
}
MX_D float warp_value(const float *src, int sh, int sw, const double *M, float cval, int x, int y) {
  int ad, bd, X0, Y0;
  warp_xterm(M, x, ad, bd);
  warp_yterm(M, y, X0, Y0);
  return warp_fetch(src, sh, sw, cval, ad, bd, X0, Y0);
}
MX_D void warp_body(const WarpJob &jb, int x, int y) {
  if (x >= jb.dcols || y >= jb.drows) return;
  jb.dst[(size_t)y * jb.dcols + x] = warp_value(jb.src, jb.srows, jb.scols, jb.M, jb.cval, x, y);
}
__global__ __launch_bounds__(256) void k_warp_affine(WarpJob jb) {
  warp_body(jb, blockIdx.x * 64 + (threadIdx.x & 63), blockIdx.y * 4 + (threadIdx.x >> 6));
}

MX_D int reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; }
  return p;
}

// one pass of a separable Gaussian with BORDER_REFLECT_101: pass 0 = rows (RowFilter / SymmRowSmallFilter order),
// pass 1 = columns (SymmColumnFilter order)
MX_D int border_idx(int p, int n, int border) {
  if (border) return p < 0 ? 0 : (p > n - 1 ? n - 1 : p);
  return reflect101(p, n);
}
MX_D void blur_body(const float *src, float *dst, int rows, int cols, const float *taps, int n, int pass, int x, int y, int border = 0) {
  if (x >= cols || y >= rows) return;
  const int R = n >> 1;
  float v;
  if (n == 1) v = src[(size_t)y * cols + x];
  else if (pass == 0) {
    const float *row = src + (size_t)y * cols;
    if (n <= 5) {
      v = row[x] * taps[R];
      for (int j = 1; j <= R; j++) v = v + (row[border_idx(x - j, cols, border)] + row[border_idx(x + j, cols, border)]) * taps[R + j];
    } else {
      v = 0.f;
      for (int j = 0; j < n; j++) v = v + row[border_idx(x + j - R, cols, border)] * taps[j];
    }
  } else {
    v = taps[R] * src[(size_t)y * cols + x] + 0.f;
    for (int j = 1; j <= R; j++)
      v = v + taps[R + j] * (src[(size_t)border_idx(y + j, rows, border) * cols + x] + src[(size_t)border_idx(y - j, rows, border) * cols + x]);
  }
  dst[(size_t)y * cols + x] = v;
}
__global__ __launch_bounds__(256) void k_blur_pass(const float *src, float *dst, int rows, int cols, const float *taps,
                                                   int n, int pass, int border) {
  blur_body(src, dst, rows, cols, taps, n, pass, blockIdx.x * 64 + (threadIdx.x & 63), blockIdx.y * 4 + (threadIdx.x >> 6), border);
}

// ---- detector responses other than the Hessian (ScaleSpaceDetector::Response, pyramid.cpp:132-175) -------------------------
// dogResponse (:176-181): in - blur(in).   computeGradient (helpers.cpp:779-797) + the three products of HarrisResponse
// (:283-305).   harris_combine: dx2 = sigmasq * blur(LxLx) ..., R = (dx2 dy2 - dxdy dxdy) - (0.04f (dx2 + dy2)) (dx2 + dy2).
__global__ __launch_bounds__(256) void k_sub(const float *a, const float *b, float *o, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) o[i] = a[i] - b[i];
}
__global__ __launch_bounds__(256) void k_grad_products(const float *img, int rows, int cols, float *xx, float *yy, float *xy) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (c >= cols || r >= rows) return;
  const float *R = img + (size_t)r * cols;
  float xg, yg;
  if (cols == 1) xg = 0.f;
  else if (c == 0) xg = R[c + 1] - R[c];
  else if (c == cols - 1) xg = R[c] - R[c - 1];
  else xg = R[c + 1] - R[c - 1];
  if (rows == 1) yg = 0.f;
  else if (r == 0) yg = R[cols + c] - R[c];
  else if (r == rows - 1) yg = R[c] - R[c - cols];
  else yg = R[cols + c] - R[c - cols];
  const size_t i = (size_t)r * cols + c;
  xx[i] = xg * xg; yy[i] = yg * yg; xy[i] = xg * yg;
}
__global__ __launch_bounds__(256) void k_harris_combine(const float *bxx, const float *byy, const float *bxy, float sigmasq, float *o, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float dx2 = bxx[i] * sigmasq, dy2 = byy[i] * sigmasq, dxdy = bxy[i] * sigmasq;
  const float s = dx2 + dy2;
  const float a = dx2 * dy2, b = dxdy * dxdy, c = (0.04f * s) * s;
  o[i] = (a - b) - c;
}

// ---- batched form: all views of a launch set in a few launches -----------------------------------------------------------------
// A view of tilt t is 1/t of the image, 31 to 61 of them per image: launched one by one they are ~250 launches of 2-10 us
// per pair.  Every block takes one tile of one view; the view is found from the tile prefix carried by the jobs.  A set is at
// most four tile lists: 64 x 4 tiles of the rotated images (rotate, blur rows, blur columns as separate launches: views whose
// filters outgrow the LDS tiles, or without a blur), 64 x 4 tiles of the outputs (tilt / zoom of those and of the next list),
// VF_TW x VF_TH tiles of k_views_rotblur (rotate + blur in one launch: a tilt that is not diagonal) and the VF_TW x VF_TH
// tiles of k_views_fused (source image to tilted view in ONE launch: every view of the shipped view sets).
// The last view whose first tile is <= `tile` (views without tiles in a list share their successor's prefix), by bisection: the
// loads depend on each other, and a walk over 30 views cost every workgroup microseconds before its first pixel.
MX_D int find_view(const ViewJob *jobs, int n, int tile, int stage) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const ViewJob &m = jobs[mid];
    const int first = stage == 3 ? m.tileG : (stage == 2 ? m.tileF : (stage ? m.tileB : m.tileA));
    if (tile >= first) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__global__ __launch_bounds__(256) void k_views_warp(const ViewJob *jobs, int n, int stage) {
  const int j = find_view(jobs, n, blockIdx.x, stage);
  const ViewJob &v = jobs[j];
  WarpJob jb;
  if (stage == 0) { jb.src = v.src; jb.dst = v.rot; jb.srows = v.srows; jb.scols = v.scols; jb.drows = v.rrows; jb.dcols = v.rcols; }
  else { jb.src = v.rot; jb.dst = v.dst; jb.srows = v.rrows; jb.scols = v.rcols; jb.drows = v.drows; jb.dcols = v.dcols; }
#pragma unroll
  for (int i = 0; i < 6; i++) jb.M[i] = stage ? v.W[i] : v.R[i];
  jb.cval = 128.f;
  const int t = blockIdx.x - (stage ? v.tileB : v.tileA), tx = (jb.dcols + 63) / 64;
  warp_body(jb, (t % tx) * 64 + (threadIdx.x & 63), (t / tx) * 4 + (threadIdx.x >> 6));
}
__global__ __launch_bounds__(256) void k_views_blur(const ViewJob *jobs, int n, const float *taps, int pass) {
  const int j = find_view(jobs, n, blockIdx.x, 0);
  const ViewJob &v = jobs[j];
  if (!v.doBlur) return;
  const int t = blockIdx.x - v.tileA, tx = (v.rcols + 63) / 64;
  const float *src = pass ? v.tmp : v.rot;
  float *dst = pass ? v.rot : v.tmp;
  blur_body(src, dst, v.rrows, v.rcols, taps + v.tapOfs + (pass ? v.kx : 0), pass ? v.ky : v.kx, pass, (t % tx) * 64 + (threadIdx.x & 63),
            (t / tx) * 4 + (threadIdx.x >> 6));
}

// One output of the row filter / the column filter over an LDS tile; N = compile-time tap count (0: runtime nx / ny), k = the
// taps in registers (N > 0), `row` / `col` = the line of the output pixel.  Terms and order are blur_body's.
template <int N>
MX_D float vf_row_value(const float *row, int lx, const float *k, const float *kxT, int Rx, int nx) {
  float r;
  if (N == 1) r = row[lx];
  else if (N == 3 || N == 5) {
    constexpr int R = N >> 1;
    r = row[lx] * k[R];
#pragma unroll
    for (int q = 1; q <= R; q++) r = r + (row[lx - q] + row[lx + q]) * k[R + q];
  } else if (N > 5) {
    constexpr int R = N >> 1;
    r = 0.f;
#pragma unroll
    for (int q = 0; q < N; q++) r = r + row[lx + q - R] * k[q];
  } else {
    if (nx <= 5) {
      r = row[lx] * kxT[Rx];
      for (int q = 1; q <= Rx; q++) r = r + (row[lx - q] + row[lx + q]) * kxT[Rx + q];
    } else {
      r = 0.f;
      for (int q = 0; q < nx; q++) r = r + row[lx + q - Rx] * kxT[q];
    }
  }
  return r;
}
template <int N>
MX_D float vf_col_value(const float *col, int lx, int stride, const float *k, const float *kyT, int Ry) {
  float r;
  if (N == 1) r = col[lx];
  else if (N > 1) {
    constexpr int R = N >> 1;
    r = k[R] * col[lx] + 0.f;
#pragma unroll
    for (int q = 1; q <= R; q++) r = r + k[R + q] * (col[lx + q * stride] + col[lx - q * stride]);
  } else {
    r = kyT[Ry] * col[lx] + 0.f;
    for (int q = 1; q <= Ry; q++) r = r + kyT[Ry + q] * (col[lx + q * stride] + col[lx - q * stride]);
  }
  return r;
}

// the two filter passes of k_views_rotblur over its LDS tiles
template <int N>
MX_D void vf_rows(const float *Wt, float *Tt, const float *kxT, int WW, int Rx, int lane, int ty, int xOut, int yEnd, int nxRt) {
  constexpr int NK = N ? N : 1;
  float k[NK];
#pragma unroll
  for (int q = 0; q < NK; q++) k[q] = N ? kxT[q] : 0.f;
  for (int ly = ty; ly < yEnd; ly += 4) {
    const float *row = Wt + ly * WW + Rx;
    for (int lx = lane; lx < xOut; lx += 64) Tt[ly * VF_TW + lx] = vf_row_value<N>(row, lx, k, kxT, Rx, nxRt);
  }
}
template <int N>
MX_D void vf_cols(const float *Tt, float *outBase, const float *kyT, int rcols, int Ry, int lane, int ty, int xOut, int yOut, int nyRt) {
  constexpr int NK = N ? N : 1;
  float k[NK];
#pragma unroll
  for (int q = 0; q < NK; q++) k[q] = N ? kyT[q] : 0.f;
  (void)nyRt;
  for (int ly = ty; ly < yOut; ly += 4) {
    const float *col = Tt + (ly + Ry) * VF_TW;
    float *out = outBase + (size_t)ly * rcols;
    for (int lx = lane; lx < xOut; lx += 64) out[lx] = vf_col_value<N>(col, lx, VF_TW, k, kyT, Ry);
  }
}

// Rotate + anti-alias blur of a view in ONE launch.  The three-launch form writes the rotated image, reads it for the row
// filter, writes the row-filtered image, reads it for the column filter and writes the result over the rotated image: four
// passes over 1-2 Mpx per view, 16-31 views per image, in kernels that wait on memory.  Here a workgroup owns a
// VF_TW x VF_TH tile of the blurred rotated image: it evaluates cv::warpAffine at the tile's pixels plus the halo the two
// filters reach (BORDER_REFLECT_101 of the ROTATED image: a halo pixel outside it is the rotation evaluated at the mirrored
// coordinate, the value the separate launches read back), filters the rows of all TH + 2 Ry lines in LDS, then the columns,
// and stores the tile.  Every value is the same f32 the separate launches pass through memory; sums, terms and order are
// those of blur_body.
__global__ __launch_bounds__(256) void k_views_rotblur(const ViewJob *jobs, int n, const float *taps, int wFloats) {
  extern __shared__ float smem[];
  const int j = find_view(jobs, n, blockIdx.x, 2);
  const ViewJob &v = jobs[j];
  const int Rx = v.kx >> 1, Ry = v.ky >> 1;
  const int t = blockIdx.x - v.tileF, tx = (v.rcols + VF_TW - 1) / VF_TW;
  const int x0 = (t % tx) * VF_TW, y0 = (t / tx) * VF_TH;
  const int WW = VF_TW + 2 * Rx;
  float *const Wt = smem, *const Tt = smem + wFloats;
  const int lane = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int xEnd = min(VF_TW, v.rcols - x0) + 2 * Rx, yEnd = min(VF_TH, v.rrows - y0) + 2 * Ry;   // what the tile's outputs reach
  {
    constexpr int NX = (VF_TW + 2 * VF_RX + 63) / 64;   // columns of the haloed tile per lane
    int ad[NX], bd[NX];
#pragma unroll
    for (int u = 0; u < NX; u++) warp_xterm(v.R, reflect101(x0 - Rx + lane + 64 * u, v.rcols), ad[u], bd[u]);
    for (int ly = ty; ly < yEnd; ly += 4) {
      int X0, Y0;
      warp_yterm(v.R, reflect101(y0 - Ry + ly, v.rrows), X0, Y0);
#pragma unroll
      for (int u = 0; u < NX; u++) {
        const int lx = lane + 64 * u;
        if (lx < xEnd) Wt[ly * WW + lx] = warp_fetch(v.src, v.srows, v.scols, 128.f, ad[u], bd[u], X0, Y0);
      }
    }
  }
  __syncthreads();
  const float *kxT = taps + v.tapOfs, *kyT = kxT + v.kx;
  const int nx = v.kx, ny = v.ky, xOut = xEnd - 2 * Rx, yOut = yEnd - 2 * Ry;
  // The filter sizes of a view are wave-uniform and small (3 .. 13 taps for every default view): one switch per pass picks a
  // fully unrolled body with the taps in registers; other sizes take the runtime loop.  Terms and order are blur_body's.
  switch (nx) {
    case 1: vf_rows<1>(Wt, Tt, kxT, WW, Rx, lane, ty, xOut, yEnd, nx); break;
    case 3: vf_rows<3>(Wt, Tt, kxT, WW, Rx, lane, ty, xOut, yEnd, nx); break;
    case 5: vf_rows<5>(Wt, Tt, kxT, WW, Rx, lane, ty, xOut, yEnd, nx); break;
    case 7: vf_rows<7>(Wt, Tt, kxT, WW, Rx, lane, ty, xOut, yEnd, nx); break;
    case 9: vf_rows<9>(Wt, Tt, kxT, WW, Rx, lane, ty, xOut, yEnd, nx); break;
    case 11: vf_rows<11>(Wt, Tt, kxT, WW, Rx, lane, ty, xOut, yEnd, nx); break;
    case 13: vf_rows<13>(Wt, Tt, kxT, WW, Rx, lane, ty, xOut, yEnd, nx); break;
    default: vf_rows<0>(Wt, Tt, kxT, WW, Rx, lane, ty, xOut, yEnd, nx); break;
  }
  __syncthreads();
  float *const outBase = v.rot + (size_t)y0 * v.rcols + x0;
  switch (ny) {
    case 1: vf_cols<1>(Tt, outBase, kyT, v.rcols, Ry, lane, ty, xOut, yOut, ny); break;
    case 3: vf_cols<3>(Tt, outBase, kyT, v.rcols, Ry, lane, ty, xOut, yOut, ny); break;
    case 5: vf_cols<5>(Tt, outBase, kyT, v.rcols, Ry, lane, ty, xOut, yOut, ny); break;
    default: vf_cols<0>(Tt, outBase, kyT, v.rcols, Ry, lane, ty, xOut, yOut, ny); break;
  }
}

// ---- source image to tilted view in ONE launch ---------------------------------------------------------------------------------
// The second cv::warpAffine of a view (tilt / zoom) has a diagonal inverse map: output column x taps the blurred columns sx(x)
// and sx(x) + 1 whatever the row, output row y the rows sy(y) and sy(y) + 1, and sx, sy are monotone.  At tilt t only 2 / t of
// the blurred columns are ever read.  k_views_rotblur + k_views_warp filter all of them, write the blurred plane (4 - 5 x the
// size of the output) and read it back; here a workgroup keeps its VF_TW x VF_TH tile of the rotated image in LDS, row-filters
// only the columns some output pixel of the tile taps, forms the column-filtered value under each tap of an output pixel in
// registers, and emits the output pixels whose (clamped) tap origin lies in the tile.  Every value is the f32 the separate
// launches pass through memory: the rotation is warp_fetch, the filter terms are vf_row_value / vf_col_value, the output is
// warp_fetch's expression over those values (warp_fetch_tile).  The rotated tile is left as it is, so the views of a launch
// set that share the rotation (a ladder step's tilts have most angles in common) are served from one rotation of the tile.
constexpr int VG_TS = VF_TW + 1;          // row stride of the row-filtered tile: the tile's columns and the one the taps sx + 1 reach
constexpr int VG_HR = VF_TH + 2 * VF_RY + 1;   // most rows of the rotated tile
constexpr int VG_TABS = VF_TW + 4;        // bytes of the tapped-column list

// tap origin of output column p (axis 0) / row p (axis 1) under a diagonal inverse map: warp_fetch's sx / sy
MX_D int warp_tap0(const double *M, int axis, int p) {
  int ad, bd, X0, Y0;
  warp_xterm(M, axis ? 0 : p, ad, bd);
  warp_yterm(M, axis ? p : 0, X0, Y0);
  const int s = ((axis ? Y0 + bd : X0 + ad) >> 5) >> 5;
  return s < -32768 ? -32768 : (s > 32767 ? 32767 : s);
}
// first p of [0, n] whose tap origin, clamped into [0, lim), reaches `target`.  The origin is monotone in p (M[0], M[4] > 0);
// `inv` only says where to start looking, the answer comes from the fixed-point map itself.
MX_D int first_reaching(const double *M, int axis, int target, int n, int lim, double inv) {
  if (target <= 0) return 0;
  if (target >= lim) return n;
  const double h = ((double)target - M[axis ? 5 : 2]) * inv;
  int p = h > 0. ? (h < (double)n ? (int)h : n) : 0;
  while (p > 0 && warp_tap0(M, axis, p - 1) >= target) p--;      // 0 < target < lim: clamping changes neither comparison
  while (p < n && warp_tap0(M, axis, p) < target) p++;
  return p;
}
// warp_fetch on the blurred tile whose origin is (x0, y0) of the sh x sw rotated image, B(r, c) = the blurred value at tile row r,
// column c: the same four products in the same order and the same three branches; a tap inside the image is in the tile for
// every pixel the tile owns
template <class Blurred>
MX_D float warp_fetch_tile(const Blurred &B, int x0, int y0, int sh, int sw, float cval, int adelta, int bdelta, int X0, int Y0) {
  const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
  int sx = X >> 5, sy = Y >> 5;
  sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
  sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
  const float fx = (float)(X & 31) * (1.f / 32), fy = (float)(Y & 31) * (1.f / 32);
  const float w0 = (1.f - fy) * (1.f - fx), w1 = (1.f - fy) * fx, w2 = fy * (1.f - fx), w3 = fy * fx;
  const int r = sy - y0, c = sx - x0;
  float out;
  if (sx >= 0 && sx < sw - 1 && sy >= 0 && sy < sh - 1) {
    const float s0 = B(r, c), s1 = B(r, c + 1), s2 = B(r + 1, c), s3 = B(r + 1, c + 1);
    out = s0 * w0 + s1 * w1 + s2 * w2 + s3 * w3;
  } else if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
    out = cval;
  } else {
    const bool bx0 = sx >= 0 && sx < sw, bx1 = sx + 1 >= 0 && sx + 1 < sw, by0 = sy >= 0 && sy < sh, by1 = sy + 1 >= 0 && sy + 1 < sh;
    const float v0 = (bx0 && by0) ? B(r, c) : cval;
    const float v1 = (bx1 && by0) ? B(r, c + 1) : cval;
    const float v2 = (bx0 && by1) ? B(r + 1, c) : cval;
    const float v3 = (bx1 && by1) ? B(r + 1, c + 1) : cval;
    out = v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3;
  }
  return out;
}
// The workgroup's 256 threads walk an (outer x inner) index space row-major: a tile of tilt 8 owns 16 output columns and taps
// 32 blurred ones, so lanes mapped to columns would idle.  One division per thread and pass.
struct FlatWalk {
  int o, i, dq, dr, n;
  MX_D FlatWalk(int tid, int inner) : o(tid / inner), i(tid - (tid / inner) * inner), dq(256 / inner), dr(256 - (256 / inner) * inner), n(inner) {}
  MX_D void next() { o += dq; i += dr; if (i >= n) { i -= n; o++; } }
};
// row filter of one view of the group at its tapped columns: Wt = the group's rotated tile (stride WW, halo gRx x gRy), of
// which the view reads the rows from dRy = gRy - Ry on; Tt row o = row y0 - Ry + o of the rotated image
template <int N>
MX_D void vg_rows(const float *Wt, float *Tt, const unsigned char *colTab, const float *kxT, int WW, int gRx, int dRy, int Rx, int tid, int nix,
                  int yEnd, int nxRt) {
  constexpr int NK = N ? N : 1;
  float k[NK];
#pragma unroll
  for (int q = 0; q < NK; q++) k[q] = N ? kxT[q] : 0.f;
  for (FlatWalk w(tid, nix); w.o < yEnd; w.next()) {
    const int lc = colTab[w.i];
    if (lc != 255) Tt[w.o * VG_TS + lc] = vf_row_value<N>(Wt + (w.o + dRy) * WW + gRx, lc, k, kxT, Rx, nxRt);
  }
}
// column filter + tilt of one view: the blurred value under each of an output pixel's four taps is formed in registers, straight
// from the row-filtered tile (vf_col_value, the call the blurred tile used to be filled by), so the rotated tile stays as it is
// for the next view of the group
template <int N>
MX_D void vg_out(const float *Tt, const ViewJob &u, const float *kyT, int Ry, int tid, int x0, int y0, int xa, int ya, int nox, int noy) {
  constexpr int NK = N ? N : 1;
  float k[NK];
#pragma unroll
  for (int q = 0; q < NK; q++) k[q] = N ? kyT[q] : 0.f;
  const auto B = [&](int lr, int lc) { return vf_col_value<N>(Tt + (lr + Ry) * VG_TS, lc, VG_TS, k, kyT, Ry); };
  for (FlatWalk w(tid, nox); w.o < noy; w.next()) {
    const int x = xa + w.i, y = ya + w.o;
    int ad, bd, X0, Y0;
    warp_xterm(u.W, x, ad, bd);
    warp_yterm(u.W, y, X0, Y0);
    u.dst[(size_t)y * u.dcols + x] = warp_fetch_tile(B, x0, y0, u.rrows, u.rcols, 128.f, ad, bd, X0, Y0);
  }
}
// A workgroup takes one tile position of a GROUP of views that share a rotation (same source, sizes and R: engine_views.hip):
// it rotates the tile once, with the widest halo of the group, and then runs the filters and the tilt of every view that owns
// an output pixel there.  The value of the rotated image at a coordinate does not depend on which view asks for it.
// (SGPRs held to what eight waves per SIMD allow: LDS admits eight workgroups per CU, and the kernel waits on the rotation's gathers)
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96))) void k_views_fused(const ViewJob *jobs, int n, const float *taps, int wFloats, int tFloats) {
  extern __shared__ float smem[];
  const ViewJob &last = jobs[find_view(jobs, n, blockIdx.x, 3)];     // the views of a group share tileG: the bisection ends at the last
  const ViewJob *const grp = jobs + last.grpFirst;
  const ViewJob &v = grp[0];                                          // what the group shares: src, sizes, R, tileG
  const int cnt = min(last.grpCount, VIEW_GROUP_CAP), gRx = last.grpRx, gRy = last.grpRy;
  const int t = blockIdx.x - v.tileG, tx = (v.rcols + VF_TW - 1) / VF_TW;
  const int x0 = (t % tx) * VF_TW, y0 = (t / tx) * VF_TH;
  const int x1 = min(x0 + VF_TW, v.rcols), y1 = min(y0 + VF_TH, v.rrows);
  const int tid = threadIdx.x;
  // Ownership: output pixel (x, y) belongs to the tile that holds (clamp(sx, 0, rcols - 1), clamp(sy, 0, rrows - 1)), so pixels
  // whose taps fall outside the rotated image are written exactly once too.  Columns [xa, xb) x rows [ya, yb) per view.
  // (each of the four waves finds one of the four bounds, view after view)
  __shared__ int own[VIEW_GROUP_CAP][4];
  {
    const int axis = tid >> 7, upper = (tid >> 6) & 1;
    for (int m = 0; m < cnt; m++) {
      const ViewJob &u = grp[m];
      const int r = first_reaching(u.W, axis, axis ? (upper ? y1 : y0) : (upper ? x1 : x0), axis ? u.drows : u.dcols, axis ? v.rrows : v.rcols, u.invW[axis]);
      if ((tid & 63) == 0) own[m][tid >> 6] = r;
    }
  }
  __syncthreads();
  {
    bool any = false;
    for (int m = 0; m < cnt; m++) any = any || (own[m][1] > own[m][0] && own[m][3] > own[m][2]);
    if (!any) return;
  }
  // blurred pixels the taps of owned pixels can read: the tile and, inside the image, the column and row behind it
  const int colsB = x1 - x0 + (x1 < v.rcols ? 1 : 0), rowsB = y1 - y0 + (y1 < v.rrows ? 1 : 0);
  const int WW = VF_TW + 2 * gRx + 1;
  float *const Wt = smem, *const Tt = smem + wFloats;          // rotated tile of the group, row-filtered tile of one view
  unsigned char *const colTab = (unsigned char *)(smem + wFloats + tFloats);
  {
    // cv::warpAffine's per-column and per-row terms of the rotation, tabulated once (they live where the row-filtered tile
    // goes afterwards); halo pixels outside the rotated image mirror it (BORDER_REFLECT_101 of the blur)
    const int xEnd = colsB + 2 * gRx, yEnd = rowsB + 2 * gRy;  // what the two filters of the group reach of the rotated image
    int *const colAd = (int *)Tt, *const colBd = colAd + WW, *const rowX0 = colBd + WW, *const rowY0 = rowX0 + VG_HR;
    for (int i = tid; i < xEnd + yEnd; i += 256) {
      if (i < xEnd) warp_xterm(v.R, reflect101(x0 - gRx + i, v.rcols), colAd[i], colBd[i]);
      else warp_yterm(v.R, reflect101(y0 - gRy + i - xEnd, v.rrows), rowX0[i - xEnd], rowY0[i - xEnd]);
    }
    __syncthreads();
    for (FlatWalk w(tid, xEnd); w.o < yEnd; w.next())
      Wt[w.o * WW + w.i] = warp_fetch(v.src, v.srows, v.scols, 128.f, colAd[w.i], colBd[w.i], rowX0[w.o], rowY0[w.o]);
  }
  __syncthreads();
  for (int m = 0; m < cnt; m++) {
    const int xa = own[m][0], xb = own[m][1], ya = own[m][2], yb = own[m][3];
    const int nox = xb - xa, noy = yb - ya;
    if (nox <= 0 || noy <= 0) continue;                        // (uniform: the whole workgroup skips the view)
    const ViewJob &u = grp[m];
    const int Rx = u.kx >> 1, Ry = u.ky >> 1;
    const int yEnd = rowsB + 2 * Ry;
    // The columns to filter: every one of the tile when the owned pixels tap at least that many (a tilt below 2), else the two
    // taps of each owned column.  255 = a tap outside the image (it reads cval, not a blurred value).  All rows the column
    // filter reaches are row-filtered.
    const bool denseX = 2 * nox >= colsB;
    const int nix = denseX ? colsB : 2 * nox;
    for (int i = tid; i < nix; i += 256) {
      const int lc = denseX ? i : warp_tap0(u.W, 0, xa + (i >> 1)) + (i & 1) - x0;
      colTab[i] = (unsigned char)(lc >= 0 && lc < colsB ? lc : 255);
    }
    __syncthreads();
    const float *kxT = taps + u.tapOfs, *kyT = kxT + u.kx;
    const int nx = u.kx, ny = u.ky;
    // wave-uniform tap counts: one switch per pass picks a fully unrolled body with the taps in registers (as k_views_rotblur)
    switch (nx) {
      case 1: vg_rows<1>(Wt, Tt, colTab, kxT, WW, gRx, gRy - Ry, Rx, tid, nix, yEnd, nx); break;
      case 3: vg_rows<3>(Wt, Tt, colTab, kxT, WW, gRx, gRy - Ry, Rx, tid, nix, yEnd, nx); break;
      case 5: vg_rows<5>(Wt, Tt, colTab, kxT, WW, gRx, gRy - Ry, Rx, tid, nix, yEnd, nx); break;
      case 7: vg_rows<7>(Wt, Tt, colTab, kxT, WW, gRx, gRy - Ry, Rx, tid, nix, yEnd, nx); break;
      case 9: vg_rows<9>(Wt, Tt, colTab, kxT, WW, gRx, gRy - Ry, Rx, tid, nix, yEnd, nx); break;
      case 11: vg_rows<11>(Wt, Tt, colTab, kxT, WW, gRx, gRy - Ry, Rx, tid, nix, yEnd, nx); break;
      case 13: vg_rows<13>(Wt, Tt, colTab, kxT, WW, gRx, gRy - Ry, Rx, tid, nix, yEnd, nx); break;
      default: vg_rows<0>(Wt, Tt, colTab, kxT, WW, gRx, gRy - Ry, Rx, tid, nix, yEnd, nx); break;
    }
    __syncthreads();
    switch (ny) {
      case 1: vg_out<1>(Tt, u, kyT, Ry, tid, x0, y0, xa, ya, nox, noy); break;
      case 3: vg_out<3>(Tt, u, kyT, Ry, tid, x0, y0, xa, ya, nox, noy); break;
      case 5: vg_out<5>(Tt, u, kyT, Ry, tid, x0, y0, xa, ya, nox, noy); break;
      default: vg_out<0>(Tt, u, kyT, Ry, tid, x0, y0, xa, ya, nox, noy); break;
    }
    __syncthreads();                                           // the next view overwrites the row-filtered tile and the column list
  }
}

void launch_warp_affine(hipStream_t s, const WarpJob &jb) {
  dim3 grid((jb.dcols + 63) / 64, (jb.drows + 3) / 4);
  hipLaunchKernelGGL(k_warp_affine, grid, dim3(256), 0, s, jb);
}
void launch_blur_pass(hipStream_t s, const float *src, float *dst, int rows, int cols, const float *taps, int n, int pass, int border) {
  dim3 grid((cols + 63) / 64, (rows + 3) / 4);
  hipLaunchKernelGGL(k_blur_pass, grid, dim3(256), 0, s, src, dst, rows, cols, taps, n, pass, border);
}
void launch_sub(hipStream_t s, const float *a, const float *b, float *o, size_t n) {
  hipLaunchKernelGGL(k_sub, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, o, n);
}
void launch_grad_products(hipStream_t s, const float *img, int rows, int cols, float *xx, float *yy, float *xy) {
  hipLaunchKernelGGL(k_grad_products, dim3((cols + 63) / 64, (rows + 3) / 4), dim3(256), 0, s, img, rows, cols, xx, yy, xy);
}
void launch_harris_combine(hipStream_t s, const float *bxx, const float *byy, const float *bxy, float sigmasq, float *o, size_t n) {
  hipLaunchKernelGGL(k_harris_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bxx, byy, bxy, sigmasq, o, n);
}
void launch_views_warp(hipStream_t s, const ViewJob *jobs, int n, int tiles, int stage) {
  if (tiles > 0) MX_DUP(K_WARP) hipLaunchKernelGGL(k_views_warp, dim3(tiles), dim3(256), 0, s, jobs, n, stage);
}
void launch_views_blur(hipStream_t s, const ViewJob *jobs, int n, int tiles, const float *taps, int pass) {
  if (tiles > 0) hipLaunchKernelGGL(k_views_blur, dim3(tiles), dim3(256), 0, s, jobs, n, taps, pass);
}
void launch_views_rotblur(hipStream_t s, const ViewJob *jobs, int n, int tiles, const float *taps, int maxRx, int maxRy) {
  if (tiles <= 0) return;
  const int wFloats = (VF_TH + 2 * maxRy) * (VF_TW + 2 * maxRx), tFloats = (VF_TH + 2 * maxRy) * VF_TW;
  MX_DUP(K_VIEW_BLUR) hipLaunchKernelGGL(k_views_rotblur, dim3(tiles), dim3(256), (size_t)(wFloats + tFloats) * 4, s, jobs, n, taps, wFloats);
}
void launch_views_fused(hipStream_t s, const ViewJob *jobs, int n, int tiles, const float *taps, int maxRx, int maxRy) {
  if (tiles <= 0) return;
  const int wFloats = (VF_TH + 2 * maxRy + 1) * (VF_TW + 2 * maxRx + 1), tFloats = (VF_TH + 2 * maxRy + 1) * VG_TS;
  static_assert(2 * (VF_TW + 2 * VF_RX + 1) + 2 * VG_HR <= (VF_TH + 1) * VG_TS, "the rotation's column / row terms fit the row-filtered tile");
  static_assert(VF_TW + 1 < 255, "tapped columns are listed as bytes");
  MX_DUP(K_VIEW_BLUR) hipLaunchKernelGGL(k_views_fused, dim3(tiles), dim3(256), (size_t)(wFloats + tFloats) * 4 + ((VG_TABS + 3) & ~3), s, jobs, n, taps,
                                         wFloats, tFloats);
}

}  // namespace mx
