// kernels_clahe.hip -- CLAHE_Impl::apply of OpenCV 2.4.9 (modules/imgproc/src/clahe.cpp) on the gray f32 image, and the rule of
// OpenCV 3.x / 4.x as variant 1.  The contract is restated in include/modsx.h; the shapes here:
//
//   k_clahe_hist   one workgroup per (image, tile, row strip).  The tile is a rectangle of the LUT source, which is the image
//                  padded at the bottom and the right with BORDER_REFLECT_101: the padding is resolved by index (a reflected row is
//                  a row of the image, a reflected column a single pixel), no padded copy exists.  The part of a tile row that lies
//                  inside the image is read as quads of four consecutive pixels (16 bytes, where the image base allows it; the
//                  ragged ends of a row as scalars), converted to bytes and counted with integer LDS atomics into one histogram
//                  per wavefront; the four are added and stored as the strip's partial [256] counts.  Integer sums: the order of
//                  the atomics does not matter.  No global atomics, nothing to clear beforehand.
//   k_clahe_lut    one wavefront per (image, tile), lane l owning bins 4l .. 4l + 3: sums the strip partials, clips, reduces the
//                  clipped count over the wave, redistributes per variant, scans the 256 bins (four in the lane, the lane totals
//                  across the wave) and rounds (float)sum * lutScale with the round-to-nearest-even convert.  256 bytes per tile.
//   k_clahe_apply  one workgroup per CLAHE_APPLY_PX consecutive pixels of an image.  The image's LUT table is copied to LDS once;
//                  a lane takes four consecutive pixels (one 16-byte load and store), the row terms ty1, ty2, ya are formed when
//                  the run starts and again if it crosses into the next row; the four products are added in the contract's order
//                  (-ffp-contract=off).  In place is fine: a lane reads its pixels before it writes them, no lane reads another's,
//                  and the launches that read the source as histogram input have finished (stream order).
#include "engine.hpp"

namespace mx {

constexpr int CL_T = 256;

// saturate_cast<uchar>(float): round to nearest even, clamp to 0 .. 255, NaN -> 0
static __device__ __forceinline__ unsigned clahe_u8(float v) {
  const float r = rintf(v);
  return r >= 0.0f ? (r > 255.0f ? 255u : (unsigned)r) : 0u;
}
// borderInterpolate(p, n, BORDER_REFLECT_101) for p >= 0 in closed form: the reflections about 0 and n - 1 have period 2 (n - 1)
static __device__ __forceinline__ int clahe_reflect(int p, int n) {
  if (p < n) return p;
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  const int m = p % period;
  return m < n ? m : period - m;
}

__global__ __launch_bounds__(CL_T) void k_clahe_hist(const ClaheImg *imgs, int tx, int ty, int *partials) {
  __shared__ int hist[CL_T / 64][CLAHE_BINS];
  const ClaheImg g = imgs[blockIdx.y];
  const int b = blockIdx.x;
  if (b >= tx * ty * g.strips) return;           // the grid is sized for the image of the batch with the most strips
  const int tile = b / g.strips, strip = b - tile * g.strips;
  const int tyi = tile / tx, txi = tile - tyi * tx;
  const int tid = threadIdx.x;
  int *mine = hist[tid >> 6];
  for (int w = 0; w < CL_T / 64; w++) hist[w][tid] = 0;
  __syncthreads();
  const int r0 = strip * g.stripRows;
  const int nr = min(g.tileH, r0 + g.stripRows) - r0;
  const int x0 = txi * g.tileW, y0 = tyi * g.tileH + r0;
  const int direct = max(0, min(g.cols - x0, g.tileW));   // columns of the tile inside the image
  if (direct > 0) {
    const int qpr = (direct + 3) / 4 + 1;        // quads that can touch `direct` consecutive pixels at any alignment
    for (int w = tid; w < nr * qpr; w += CL_T) {
      const int r = w / qpr, k = w - r * qpr;
      const int yy = clahe_reflect(y0 + r, g.rows);
      const int start = yy * g.cols + x0, end = start + direct;      // < rows * cols <= 2^26
      const int q = (start & ~3) + 4 * k;
      if (q >= end) continue;
      if (g.vec && q >= start && q + 4 <= end) {
        const float4 v = *reinterpret_cast<const float4 *>(g.src + q);
        atomicAdd(&mine[clahe_u8(v.x)], 1);
        atomicAdd(&mine[clahe_u8(v.y)], 1);
        atomicAdd(&mine[clahe_u8(v.z)], 1);
        atomicAdd(&mine[clahe_u8(v.w)], 1);
      } else {
        for (int j = 0; j < 4; j++) {
          const int i = q + j;
          if (i >= start && i < end) atomicAdd(&mine[clahe_u8(g.src[i])], 1);
        }
      }
    }
  }
  const int padc = g.tileW - direct;             // columns right of the image: reflected pixel by pixel
  for (int w = tid; w < nr * padc; w += CL_T) {
    const int r = w / padc, c = direct + (w - r * padc);
    const int yy = clahe_reflect(y0 + r, g.rows), xx = clahe_reflect(x0 + c, g.cols);
    atomicAdd(&mine[clahe_u8(g.src[yy * g.cols + xx])], 1);
  }
  __syncthreads();
  int sum = 0;
  for (int w = 0; w < CL_T / 64; w++) sum += hist[w][tid];
  partials[(g.partOfs + (long long)tile * g.strips + strip) * CLAHE_BINS + tid] = sum;
}

template <int VARIANT>
__global__ __launch_bounds__(64) void k_clahe_lut(const ClaheImg *imgs, const int *partials, unsigned char *lut, int *dbgHist) {
  const ClaheImg g = imgs[blockIdx.y];
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int4 *p = reinterpret_cast<const int4 *>(partials + (g.partOfs + (long long)tile * g.strips) * CLAHE_BINS) + lane;
  int h[4] = {0, 0, 0, 0};
  for (int s = 0; s < g.strips; s++) {
    const int4 v = p[s * 64];
    h[0] += v.x; h[1] += v.y; h[2] += v.z; h[3] += v.w;
  }
  if (dbgHist) reinterpret_cast<int4 *>(dbgHist + (g.lutOfs + tile) * CLAHE_BINS)[lane] = make_int4(h[0], h[1], h[2], h[3]);
  if (g.clipLimit > 0) {
    int clipped = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      clipped += max(h[k] - g.clipLimit, 0);
      h[k] = min(h[k], g.clipLimit);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) clipped += __shfl_xor(clipped, d);
    const int batch = clipped / CLAHE_BINS, residual = clipped - batch * CLAHE_BINS;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int bin = 4 * lane + k;
      h[k] += batch;
      if (VARIANT == 0) {
        if (bin < residual) h[k]++;
      } else if (residual) {
        // for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++: bins 0, step, 2 step, ...; residual < 256, so
        // step = 256 / residual >= 1 and all `residual` of them lie below 256
        const int step = CLAHE_BINS / residual;
        if (bin % step == 0 && bin / step < residual) h[k]++;
      }
    }
  }
  h[1] += h[0]; h[2] += h[1]; h[3] += h[2];
  int inc = h[3];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  const int base = inc - h[3];
  unsigned packed = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) packed |= clahe_u8((float)(base + h[k]) * g.lutScale) << (8 * k);
  reinterpret_cast<unsigned *>(lut + (g.lutOfs + tile) * CLAHE_BINS)[lane] = packed;
}

// ty1, ty2, ya of a row (or tx1, tx2, xa of a column): i = the coordinate, tile = the tile's extent, nt = tiles along the axis
template <int VARIANT>
static __device__ __forceinline__ void clahe_axis(int i, int tile, int nt, int &t1, int &t2, float &a) {
  const float f = VARIANT == 0 ? (float)i / (float)tile - 0.5f : (float)i * (1.0f / (float)tile) - 0.5f;
  const float fl = floorf(f);
  t1 = (int)fl;
  a = f - fl;
  t2 = min(t1 + 1, nt - 1);
  t1 = min(max(t1, 0), nt - 1);                  // the upper bound never binds for a coordinate inside the image; it keeps the LDS index in the table
}

template <int VARIANT>
__global__ __launch_bounds__(CL_T) void k_clahe_apply(const ClaheImg *imgs, int tx, int ty, const unsigned char *lut) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const ClaheImg g = imgs[blockIdx.y];
  if ((int)blockIdx.x >= g.applyBlocks) return;  // the grid is sized for the largest image of the batch
  const int tid = threadIdx.x;
  {
    const uint4 *L = reinterpret_cast<const uint4 *>(lut + g.lutOfs * CLAHE_BINS);
    for (int i = tid; i < tx * ty * (CLAHE_BINS / 16); i += CL_T) reinterpret_cast<uint4 *>(lds)[i] = L[i];
  }
  __syncthreads();
  const int n = g.rows * g.cols;
  const int first = blockIdx.x * CLAHE_APPLY_PX;
  for (int it = 0; it < CLAHE_APPLY_PX / (CL_T * 4); it++) {
    const int i0 = first + (it * CL_T + tid) * 4;
    if (i0 >= n) break;
    const int cnt = min(4, n - i0);
    const bool quad = g.vec && cnt == 4;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (quad) {
      const float4 q = *reinterpret_cast<const float4 *>(g.src + i0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      for (int j = 0; j < cnt; j++) v[j] = g.src[i0 + j];
    }
    int y = i0 / g.cols, x = i0 - y * g.cols;
    int ty1, ty2, tx1, tx2;
    float ya, xa;
    clahe_axis<VARIANT>(y, g.tileH, ty, ty1, ty2, ya);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (j < cnt) {
        if (x == g.cols) {                       // the run goes on in the next row
          x = 0; y++;
          clahe_axis<VARIANT>(y, g.tileH, ty, ty1, ty2, ya);
        }
        clahe_axis<VARIANT>(x, g.tileW, tx, tx1, tx2, xa);
        const unsigned s = clahe_u8(v[j]);
        const float l11 = (float)lds[(ty1 * tx + tx1) * CLAHE_BINS + s], l12 = (float)lds[(ty1 * tx + tx2) * CLAHE_BINS + s];
        const float l21 = (float)lds[(ty2 * tx + tx1) * CLAHE_BINS + s], l22 = (float)lds[(ty2 * tx + tx2) * CLAHE_BINS + s];
        float res;
        if (VARIANT == 0) {
          res = 0.0f;
          res += l11 * ((1.0f - xa) * (1.0f - ya));
          res += l12 * (xa * (1.0f - ya));
          res += l21 * ((1.0f - xa) * ya);
          res += l22 * (xa * ya);
        } else {
          const float xa1 = 1.0f - xa, ya1 = 1.0f - ya;
          res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
        }
        v[j] = (float)clahe_u8(res);
        x++;
      }
    }
    if (quad) {
      *reinterpret_cast<float4 *>(g.dst + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int j = 0; j < cnt; j++) g.dst[i0 + j] = v[j];
    }
  }
}

void launch_clahe_hist(hipStream_t s, const ClaheImg *imgs, int n, int tx, int ty, int maxStrips, int *partials) {
  hipLaunchKernelGGL(k_clahe_hist, dim3(tx * ty * maxStrips, n), dim3(CL_T), 0, s, imgs, tx, ty, partials);
}

void launch_clahe_lut(hipStream_t s, const ClaheImg *imgs, int n, int tiles, int variant, const int *partials, unsigned char *lut,
                      int *dbgHist) {
  if (variant == 0) hipLaunchKernelGGL(k_clahe_lut<0>, dim3(tiles, n), dim3(64), 0, s, imgs, partials, lut, dbgHist);
  else hipLaunchKernelGGL(k_clahe_lut<1>, dim3(tiles, n), dim3(64), 0, s, imgs, partials, lut, dbgHist);
}

void launch_clahe_apply(hipStream_t s, const ClaheImg *imgs, int n, int tx, int ty, int variant, int maxBlocks, const unsigned char *lut) {
  const size_t ldsBytes = (size_t)tx * ty * CLAHE_BINS;
  if (variant == 0) hipLaunchKernelGGL(k_clahe_apply<0>, dim3(maxBlocks, n), dim3(CL_T), ldsBytes, s, imgs, tx, ty, lut);
  else hipLaunchKernelGGL(k_clahe_apply<1>, dim3(maxBlocks, n), dim3(CL_T), ldsBytes, s, imgs, tx, ty, lut);
}

}  // namespace mx
