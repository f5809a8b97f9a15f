// kernels_surfdet.hip -- the SURF detector (OpenSURF's FastHessian) on whole views.
//
// Reference: the SURF branch                  imagerepresentation.cpp:1046-1076
//   Integral / getGray                        opensurf/integral.cpp:18-55, opensurf/utils.cpp:62-82
//   BoxIntegral                               opensurf/integral.h:35-53
//   ResponseLayer::getResponse / getLaplacian opensurf/responselayer.h:46-76
//   buildResponseLayer, isExtremum, interpolateExtremum / interpolateStep / deriv3D / hessian3D
//                                             opensurf/fasthessian.cpp:193-373
// Every kernel reads the job table (one SdJob per image) and finds its image and part through a table of workgroup runs, so a
// view set is one launch set.  Each stage keeps the reference's operations and their order (the order of f32 adds is the result):
//   k_sd_rows     g = p * (float)(1.0 / 255.0) + 0.0f and the serial running sum rs of every row.  A one-wave workgroup takes 16
//                 rows: it loads a 16 x 64 tile with coalesced row reads into LDS, lanes 0 .. 15 walk one row of the tile each
//                 (stride 65 words: no bank conflict) carrying rs from tile to tile, and the tile goes back with coalesced writes.
//   k_sd_cols     I[r][c] = rs[r][c] + I[r - 1][c]: one lane per column, 64 neighbouring columns per wave (coalesced as it is),
//                 eight rows loaded ahead of the eight dependent adds.
//                 No tree and no wave scan anywhere: they would change the bits.
//   k_sd_resp     one lane per response of any layer of any job: 8 BoxIntegrals of 4 reads of the integral image.
//   k_sd_scan     one lane per position of the t layer of every (job, octave, interval), in getIpoints' order: isExtremum, and for
//                 an extremum the sub-pixel step in f64; writes a flag byte (1 extremum, 2 accepted) and per-tile counts.
//   k_sd_offsets  exclusive scan of the tile counts (integers: any order), one workgroup.
//   k_sd_emit     the second pass: ranks the flagged lanes of a tile by ballot, repeats the sub-pixel step and stores the point (and,
//                 for the debug tap, the raw extremum with dD, H, x) at tile offset + rank -- the reference's push order, no atomics.
// The 3 x 3 inverse of interpolateStep (cvInvert with CV_SVD in the reference) is sd_inv3: the adjugate over the determinant in f64 in
// a fixed order, zeros where the determinant is 0 or not finite.
#include "engine.hpp"

namespace mx {

constexpr int SD_T = 64;
static_assert(SD_TILE % 64 == 0 && SD_TILE <= 1024, "a scan tile is a whole number of waves");

// the run that holds workgroup blk: the last one with blk0 <= blk
MX_D int sd_find(const SdSeg *__restrict__ segs, int n, int blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(SD_T) void k_sd_rows(const SdJob *__restrict__ jobs, const SdSeg *__restrict__ segs, int nsegs) {
  __shared__ float tile[SD_ROWS_PER_WG][SD_T + 1];
  const SdSeg sg = segs[sd_find(segs, nsegs, blockIdx.x)];
  const SdJob &J = jobs[sg.job];
  const int lane = threadIdx.x, rows = J.rows, cols = J.cols;
  const int r0 = (blockIdx.x - sg.blk0) * SD_ROWS_PER_WG, nr = min(SD_ROWS_PER_WG, rows - r0);
  const float *__restrict__ src = J.src;
  float *__restrict__ dst = J.integ;
  const float gscale = (float)(1.0 / 255.0), gshift = 0.0f;
  float rs = 0.0f;
  for (int c0 = 0; c0 < cols; c0 += SD_T) {
    const int nc = min(SD_T, cols - c0);
    if (lane < nc)
      for (int r = 0; r < nr; r++) tile[r][lane] = src[(size_t)(r0 + r) * cols + c0 + lane] * gscale + gshift;
    __syncthreads();
    if (lane < nr)
      for (int c = 0; c < nc; c++) { rs += tile[lane][c]; tile[lane][c] = rs; }
    __syncthreads();
    if (lane < nc)
      for (int r = 0; r < nr; r++) dst[(size_t)(r0 + r) * cols + c0 + lane] = tile[r][lane];
    __syncthreads();
  }
}

__global__ __launch_bounds__(SD_T) void k_sd_cols(const SdJob *__restrict__ jobs, const SdSeg *__restrict__ segs, int nsegs) {
  const SdSeg sg = segs[sd_find(segs, nsegs, blockIdx.x)];
  const SdJob &J = jobs[sg.job];
  const int rows = J.rows, cols = J.cols, c = (blockIdx.x - sg.blk0) * SD_T + threadIdx.x;
  if (c >= cols) return;
  float *__restrict__ I = J.integ + c;
  float above = I[0];
  int r = 1;
  for (; r + 8 <= rows; r += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = I[(size_t)(r + k) * cols];
#pragma unroll
    for (int k = 0; k < 8; k++) { above = v[k] + above; I[(size_t)(r + k) * cols] = above; }
  }
  for (; r < rows; r++) { above = I[(size_t)r * cols] + above; I[(size_t)r * cols] = above; }
}

// BoxIntegral (integral.h:35-53): std::max(0.f, v) is v only where 0.f < v
MX_D float sd_box(const float *__restrict__ I, int height, int width, int row, int col, int rows, int cols) {
  const int r1 = min(row, height) - 1, c1 = min(col, width) - 1, r2 = min(row + rows, height) - 1, c2 = min(col + cols, width) - 1;
  float A = 0.0f, B = 0.0f, C = 0.0f, D = 0.0f;
  if (r1 >= 0 && c1 >= 0) A = I[(size_t)r1 * width + c1];
  if (r1 >= 0 && c2 >= 0) B = I[(size_t)r1 * width + c2];
  if (r2 >= 0 && c1 >= 0) C = I[(size_t)r2 * width + c1];
  if (r2 >= 0 && c2 >= 0) D = I[(size_t)r2 * width + c2];
  const float v = A - B - C + D;
  return 0.f < v ? v : 0.f;
}

// buildResponseLayer (fasthessian.cpp:193-237)
__global__ __launch_bounds__(SD_TILE) void k_sd_resp(const SdJob *__restrict__ jobs, const SdSeg *__restrict__ segs, int nsegs,
                                                     float *__restrict__ resp, unsigned char *__restrict__ lapl) {
  const SdSeg sg = segs[sd_find(segs, nsegs, blockIdx.x)];
  const SdJob &J = jobs[sg.job];
  const SdLayer L = J.L[sg.a];
  const int index = (blockIdx.x - sg.blk0) * SD_TILE + threadIdx.x;
  if (index >= L.w * L.h) return;
  const int ar = index / L.w, ac = index - ar * L.w;
  const int step = L.step, b = (L.filter - 1) / 2, l = L.filter / 3, w = L.filter;
  const float inverse_area = 1.f / (w * w);
  const float *__restrict__ img = J.integ;
  const int ih = J.rows, iw = J.cols;
  const int r = ar * step, c = ac * step;
  float Dxx = sd_box(img, ih, iw, r - l + 1, c - b, 2 * l - 1, w) - sd_box(img, ih, iw, r - l + 1, c - l / 2, 2 * l - 1, l) * 3;
  float Dyy = sd_box(img, ih, iw, r - b, c - l + 1, w, 2 * l - 1) - sd_box(img, ih, iw, r - l / 2, c - l + 1, l, 2 * l - 1) * 3;
  float Dxy = +sd_box(img, ih, iw, r - l, c + 1, l, l) + sd_box(img, ih, iw, r + 1, c - l, l, l) - sd_box(img, ih, iw, r - l, c - l, l, l) -
              sd_box(img, ih, iw, r + 1, c + 1, l, l);
  Dxx *= inverse_area;
  Dyy *= inverse_area;
  Dxy *= inverse_area;
  resp[L.ofs + index] = (Dxx * Dyy - 0.81f * Dxy * Dxy);
  lapl[L.ofs + index] = (Dxx + Dyy >= 0 ? 1 : 0);
}

// the layers of (octave o, interval i) as getIpoints picks them (filter_map, fasthessian.cpp:97), read through getResponse: the scale
// of a denser layer is the integer quotient of the WIDTHS, used for rows as well (responselayer.h:67-76)
struct SdTriple {
  const float *T, *M, *B;
  const unsigned char *Ml;
  int tw, th, mw, bw, sm, sb, step, mfilter, filterStep, border;
  MX_D float t(int r, int c) const { return T[r * tw + c]; }
  MX_D float m(int r, int c) const { return M[(sm * r) * mw + (sm * c)]; }
  MX_D float b(int r, int c) const { return B[(sb * r) * bw + (sb * c)]; }
};
MX_D SdTriple sd_triple(const SdJob &J, int o, int i, const float *__restrict__ resp, const unsigned char *__restrict__ lapl) {
  constexpr int filter_map[5][4] = {{0, 1, 2, 3}, {1, 3, 4, 5}, {3, 5, 6, 7}, {5, 7, 8, 9}, {7, 9, 10, 11}};
  const SdLayer &b = J.L[filter_map[o][i]], &m = J.L[filter_map[o][i + 1]], &t = J.L[filter_map[o][i + 2]];
  SdTriple q;
  q.T = resp + t.ofs; q.M = resp + m.ofs; q.B = resp + b.ofs; q.Ml = lapl + m.ofs;
  q.tw = t.w; q.th = t.h; q.mw = m.w; q.bw = b.w;
  q.sm = m.w / t.w; q.sb = b.w / t.w;
  q.step = t.step; q.mfilter = m.filter; q.filterStep = m.filter - b.filter;
  q.border = (t.filter + 1) / (2 * t.step);
  return q;
}

// isExtremum (fasthessian.cpp:242-269)
MX_D bool sd_is_extremum(const SdTriple &q, int r, int c, float thresh) {
  if (r <= q.border || r >= q.th - q.border || c <= q.border || c >= q.tw - q.border) return false;
  const float candidate = q.m(r, c);
  if (candidate < thresh) return false;
  for (int rr = -1; rr <= 1; ++rr)
    for (int cc = -1; cc <= 1; ++cc)
      if (q.t(r + rr, c + cc) >= candidate || ((rr != 0 || cc != 0) && q.m(r + rr, c + cc) >= candidate) ||
          q.b(r + rr, c + cc) >= candidate)
        return false;
  return true;
}

// the specification of the 3 x 3 inverse: adjugate over determinant, f64, this order; zeros where the determinant is 0 or not finite
MX_D void sd_inv3(const double *S, double *t) {
  double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
  if (d == 0. || !(fabs(d) <= 1.7976931348623157e308)) { for (int i = 0; i < 9; i++) t[i] = 0; return; }
  d = 1. / d;
  t[0] = (S[4] * S[8] - S[5] * S[7]) * d; t[1] = (S[2] * S[7] - S[1] * S[8]) * d; t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
  t[3] = (S[5] * S[6] - S[3] * S[8]) * d; t[4] = (S[0] * S[8] - S[2] * S[6]) * d; t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
  t[6] = (S[3] * S[7] - S[4] * S[6]) * d; t[7] = (S[1] * S[6] - S[0] * S[7]) * d; t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
}

// interpolateExtremum / interpolateStep / deriv3D / hessian3D (fasthessian.cpp:274-373).  dD = (dx, dy, ds), Hs = (dxx, dxy, dxs, dyy,
// dys, dss), x = (xc, xr, xi); returns whether the point is accepted
MX_D bool sd_interpolate(const SdTriple &q, int r, int c, double *dD, double *Hs, double *x, SdPoint &p) {
  const double dx = (q.m(r, c + 1) - q.m(r, c - 1)) / 2.0;
  const double dy = (q.m(r + 1, c) - q.m(r - 1, c)) / 2.0;
  const double ds = (q.t(r, c) - q.b(r, c)) / 2.0;
  const double v = q.m(r, c);
  const double dxx = q.m(r, c + 1) + q.m(r, c - 1) - 2 * v;
  const double dyy = q.m(r + 1, c) + q.m(r - 1, c) - 2 * v;
  const double dss = q.t(r, c) + q.b(r, c) - 2 * v;
  const double dxy = (q.m(r + 1, c + 1) - q.m(r + 1, c - 1) - q.m(r - 1, c + 1) + q.m(r - 1, c - 1)) / 4.0;
  const double dxs = (q.t(r, c + 1) - q.t(r, c - 1) - q.b(r, c + 1) + q.b(r, c - 1)) / 4.0;
  const double dys = (q.t(r + 1, c) - q.t(r - 1, c) - q.b(r + 1, c) + q.b(r - 1, c)) / 4.0;
  const double H[9] = {dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss};
  double Hi[9];
  sd_inv3(H, Hi);
  for (int k = 0; k < 3; k++) x[k] = -1.0 * (Hi[3 * k] * dx + Hi[3 * k + 1] * dy + Hi[3 * k + 2] * ds);
  dD[0] = dx; dD[1] = dy; dD[2] = ds;
  Hs[0] = dxx; Hs[1] = dxy; Hs[2] = dxs; Hs[3] = dyy; Hs[4] = dys; Hs[5] = dss;
  const double xi = x[2], xr = x[1], xc = x[0];
  p.x = static_cast<float>((c + xc) * q.step);
  p.y = static_cast<float>((r + xr) * q.step);
  p.scale = static_cast<float>((0.1333f) * (q.mfilter + xi * q.filterStep));
  p.laplacian = q.Ml[(q.sm * r) * q.mw + (q.sm * c)];
  return fabs(xi) < 0.5f && fabs(xr) < 0.5f && fabs(xc) < 0.5f;
}

// segs: runs of SD_TILE raster positions of the t layer of (job, octave a, interval b), in getIpoints' order
__global__ __launch_bounds__(SD_TILE) void k_sd_scan(const SdJob *__restrict__ jobs, const SdSeg *__restrict__ segs, int nsegs,
                                                     const float *__restrict__ resp, const unsigned char *__restrict__ lapl, float thresh,
                                                     unsigned char *__restrict__ flags, int *__restrict__ counts) {
  const SdSeg sg = segs[sd_find(segs, nsegs, blockIdx.x)];
  const SdTriple q = sd_triple(jobs[sg.job], sg.a, sg.b, resp, lapl);
  const int index = (blockIdx.x - sg.blk0) * SD_TILE + threadIdx.x;
  int flag = 0;
  if (index < q.tw * q.th) {
    const int r = index / q.tw, c = index - r * q.tw;
    if (sd_is_extremum(q, r, c, thresh)) {
      double dD[3], Hs[6], x[3];
      SdPoint p;
      flag = sd_interpolate(q, r, c, dD, Hs, x, p) ? 3 : 1;
    }
  }
  flags[(size_t)blockIdx.x * SD_TILE + threadIdx.x] = (unsigned char)flag;
  const int nExt = __syncthreads_count(flag & 1), nAcc = __syncthreads_count(flag == 3);
  if (threadIdx.x == 0) { counts[2 * blockIdx.x] = nExt; counts[2 * blockIdx.x + 1] = nAcc; }
}

// offs [n + 1][2] = the exclusive scan of counts [n][2]; jobStart [nj + 1][2] = offs at tile0[j] (tile0[nj] = n).  One workgroup
constexpr int SD_SCAN_T = 1024;
__global__ __launch_bounds__(SD_SCAN_T) void k_sd_offsets(const int *__restrict__ counts, int n, int *__restrict__ offs,
                                                          const int *__restrict__ tile0, int nj, int *__restrict__ jobStart) {
  __shared__ int sa[SD_SCAN_T], sb[SD_SCAN_T];
  const int t = threadIdx.x, chunk = (n + SD_SCAN_T - 1) / SD_SCAN_T;
  const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
  int a = 0, b = 0;
  for (int k = lo; k < hi; k++) { a += counts[2 * k]; b += counts[2 * k + 1]; }
  sa[t] = a; sb[t] = b;
  __syncthreads();
  for (int d = 1; d < SD_SCAN_T; d <<= 1) {
    const int va = t >= d ? sa[t - d] : 0, vb = t >= d ? sb[t - d] : 0;
    __syncthreads();
    sa[t] += va; sb[t] += vb;
    __syncthreads();
  }
  int ra = sa[t] - a, rb = sb[t] - b;
  for (int k = lo; k < hi; k++) { offs[2 * k] = ra; offs[2 * k + 1] = rb; ra += counts[2 * k]; rb += counts[2 * k + 1]; }
  if (t == SD_SCAN_T - 1) { offs[2 * n] = sa[t]; offs[2 * n + 1] = sb[t]; }
  __syncthreads();
  for (int j = t; j <= nj; j += SD_SCAN_T) { jobStart[2 * j] = offs[2 * tile0[j]]; jobStart[2 * j + 1] = offs[2 * tile0[j] + 1]; }
}

__global__ __launch_bounds__(SD_TILE) void k_sd_emit(const SdJob *__restrict__ jobs, const SdSeg *__restrict__ segs, int nsegs,
                                                     const float *__restrict__ resp, const unsigned char *__restrict__ lapl,
                                                     const unsigned char *__restrict__ flags, const int *__restrict__ offs,
                                                     SdPoint *__restrict__ points, int capPts, SdExt *__restrict__ ext, int capExt) {
  __shared__ int wE[SD_TILE / 64], wA[SD_TILE / 64];
  const int flag = flags[(size_t)blockIdx.x * SD_TILE + threadIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bE = __ballot(flag & 1), bA = __ballot(flag == 3), below = (1ull << lane) - 1;
  if (lane == 0) { wE[wave] = __popcll(bE); wA[wave] = __popcll(bA); }
  __syncthreads();
  if (!(flag & 1)) return;
  int iE = offs[2 * blockIdx.x] + __popcll(bE & below), iA = offs[2 * blockIdx.x + 1] + __popcll(bA & below);
  for (int w = 0; w < wave; w++) { iE += wE[w]; iA += wA[w]; }
  const SdSeg sg = segs[sd_find(segs, nsegs, blockIdx.x)];
  const SdTriple q = sd_triple(jobs[sg.job], sg.a, sg.b, resp, lapl);
  const int index = (blockIdx.x - sg.blk0) * SD_TILE + threadIdx.x;
  const int r = index / q.tw, c = index - r * q.tw;
  SdExt e;
  SdPoint p;
  const bool ok = sd_interpolate(q, r, c, e.dD, e.H, e.x, p);
  if (ext && iE < capExt) {
    e.job = sg.job; e.o = sg.a; e.i = sg.b; e.r = r; e.c = c; e.accepted = ok ? 1 : 0; e.laplacian = p.laplacian; e.pad = 0;
    ext[iE] = e;
  }
  if (points && flag == 3 && iA < capPts) points[iA] = p;
}

void launch_surfdet_integral(hipStream_t s, const SdJob *jobs, const SdSeg *rowSegs, int nRowSegs, int rowBlocks, const SdSeg *colSegs,
                             int nColSegs, int colBlocks) {
  if (rowBlocks <= 0 || colBlocks <= 0) return;
  hipLaunchKernelGGL(k_sd_rows, dim3(rowBlocks), dim3(SD_T), 0, s, jobs, rowSegs, nRowSegs);
  hipLaunchKernelGGL(k_sd_cols, dim3(colBlocks), dim3(SD_T), 0, s, jobs, colSegs, nColSegs);
}

void launch_surfdet_responses(hipStream_t s, const SdJob *jobs, const SdSeg *segs, int nsegs, int blocks, float *resp, unsigned char *lap) {
  if (blocks <= 0) return;
  hipLaunchKernelGGL(k_sd_resp, dim3(blocks), dim3(SD_TILE), 0, s, jobs, segs, nsegs, resp, lap);
}

void launch_surfdet_scan(hipStream_t s, const SdJob *jobs, const SdSeg *segs, int nsegs, int tiles, const float *resp,
                         const unsigned char *lap, float thresh, unsigned char *flags, int *counts, int *offs, const int *tile0, int nj,
                         int *jobStart) {
  if (tiles > 0) hipLaunchKernelGGL(k_sd_scan, dim3(tiles), dim3(SD_TILE), 0, s, jobs, segs, nsegs, resp, lap, thresh, flags, counts);
  hipLaunchKernelGGL(k_sd_offsets, dim3(1), dim3(SD_SCAN_T), 0, s, counts, tiles, offs, tile0, nj, jobStart);
}

void launch_surfdet_emit(hipStream_t s, const SdJob *jobs, const SdSeg *segs, int nsegs, int tiles, const float *resp,
                         const unsigned char *lap, const unsigned char *flags, const int *offs, SdPoint *points, int capPts, SdExt *ext,
                         int capExt) {
  if (tiles <= 0) return;
  hipLaunchKernelGGL(k_sd_emit, dim3(tiles), dim3(SD_TILE), 0, s, jobs, segs, nsegs, resp, lap, flags, offs, points, capPts, ext, capExt);
}

}  // namespace mx
