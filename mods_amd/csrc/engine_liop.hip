// engine_liop.hip -- DescribeRegions<LIOPDescriptor> (synth-detection.hpp:169-255 with matching/liopdesc.hpp:55-63) and the
// normalised patches DescribeRegions<> hands to any functor, as device outputs.
//   * the tables of vl_liopdesc_new_basic(41) (vlfeat/vl/liop.c:346-395) are built here on the host, with libm as the reference
//     builds them, once per context;
//   * patches come from the description front end unchanged: the windows, the chunk planner (describe_plan.cpp) and the sampling
//     and blur launches of describe_batch, with the patch-out form of k_describe as the last launch (DescTail);
//   * a LIOP call passes its patches through a per-context buffer of at most 64 MiB: sub-batches of a chunk's jobs, patch-out
//     launch then k_liop (MODSX_LIOP_BATCH = patches per sub-batch, read once per process).
// LIOP has no parameters of its own: the ini's neighbours / bins / radius / threshold keys never reach VLFeat.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

constexpr int LIOP_SIDE = 41, LIOP_NPX = LIOP_SIDE * LIOP_SIDE, LIOP_N = MODSX_LIOP_PIXELS, LIOP_DIM = MODSX_LIOP_DIM;
constexpr size_t LIOP_PATCH_B = (size_t)LIOP_NPX * 4, LIOP_BUF_B = (size_t)64 << 20;
constexpr size_t LIOP_TAB_SAMPLES = ((size_t)LIOP_N * 2 + 7) & ~(size_t)7;      // byte offset of the sample table behind the pixels

// vl_liopdesc_new(4, 6, 6.0f, 41): the measurement pixels (raster order, the x == 0 && y == 0 skip of liop.c:355) and the four
// neighbour samples of each.  Fills the first `cap` entries; returns the number of measurement pixels.
int liop_tables(int patchSize, int *pixels, double *sx, double *sy, int cap) {
  if (patchSize != LIOP_SIDE) { set_error("LIOP: patchSize must be 41"); return MODSX_ERR_ARG; }
  const long sideLength = patchSize, center = (sideLength - 1) / 2;
  const float radius = 6.0f;
  const int numNeighbours = 4;
  const double t = center - radius + 0.6;
  const long t2 = (long)(t * t);
  int n = 0;
  for (long y = 0; y < sideLength; ++y)
    for (long x = 0; x < sideLength; ++x) {
      const long dx = x - center, dy = y - center;
      if (x == 0 && y == 0) continue;
      if (dx * dx + dy * dy > t2) continue;
      if (n < cap) {
        if (pixels) pixels[n] = (int)(x + y * sideLength);
        const double xd = (double)dx, yd = (double)dy;
        const double dangle = 2 * 3.141592653589793 / (double)numNeighbours;
        const double angle0 = atan2(yd, xd);
        for (long k = 0; k < numNeighbours; ++k) {
          const double x1 = xd + radius * cos(angle0 + dangle * k) + center;
          const double y1 = yd + radius * sin(angle0 + dangle * k) + center;
          if (sx) sx[(size_t)n * numNeighbours + k] = x1;
          if (sy) sy[(size_t)n * numNeighbours + k] = y1;
        }
      }
      n++;
    }
  return n;
}

static long vl_floor_d(double x) {      // vl/mathop.h:147-152
  const long xi = (long)x;
  if (x >= 0 || (double)xi == x) return xi;
  return xi - 1;
}

static int ensure_tables(modsx_ctx *c) {
  if (c->liopTab.p) return MODSX_OK;
  std::vector<int> pix(LIOP_N);
  std::vector<double> sx((size_t)LIOP_N * 4), sy((size_t)LIOP_N * 4);
  const int n = liop_tables(LIOP_SIDE, pix.data(), sx.data(), sy.data(), LIOP_N);
  if (n != LIOP_N) { set_error("LIOP: the measurement disc of a 41 x 41 patch has 673 pixels"); return MODSX_ERR_ARG; }
  std::vector<char> blob(LIOP_TAB_SAMPLES + (size_t)LIOP_N * 4 * sizeof(LiopSample), 0);
  unsigned short *p16 = (unsigned short *)blob.data();
  LiopSample *smp = (LiopSample *)(blob.data() + LIOP_TAB_SAMPLES);
  for (int i = 0; i < LIOP_N; i++) p16[i] = (unsigned short)pix[i];
  for (size_t i = 0; i < (size_t)LIOP_N * 4; i++) {
    const long ix = vl_floor_d(sx[i]), iy = vl_floor_d(sy[i]);
    smp[i].ix = (int)ix; smp[i].iy = (int)iy;
    smp[i].wx = sx[i] - ix; smp[i].wy = sy[i] - iy;
  }
  if (!c->liopTab.ensure(blob.size())) return MODSX_ERR_NOMEM;
  hipError_t e = hipMemcpy(c->liopTab.p, blob.data(), blob.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) { c->liopTab.release(); MX_HIP(e); }
  return MODSX_OK;
}
static const unsigned short *tab_pixels(modsx_ctx *c) { return (const unsigned short *)c->liopTab.p; }
static const LiopSample *tab_samples(modsx_ctx *c) { return (const LiopSample *)((const char *)c->liopTab.p + LIOP_TAB_SAMPLES); }

// patches per sub-batch: what fits 64 MiB, or MODSX_LIOP_BATCH (1 .. that many), read once per process
static int liop_batch() {
  static const int b = [] {
    const long full = (long)(LIOP_BUF_B / LIOP_PATCH_B);
    const char *e = getenv("MODSX_LIOP_BATCH");
    const long v = e ? atol(e) : full;
    return (int)std::min(std::max(v, 1L), full);
  }();
  return b;
}

static int zero_counter(modsx_ctx *c) {
  if (!c->liopCnt.ensure(16)) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemsetAsync(c->liopCnt.p, 0, 16, c->stream));
  return MODSX_OK;
}
static int book_call(modsx_ctx *c, int n, long subBatches) {
  unsigned cnt = 0;
  MX_HIP(hipMemcpyAsync(&cnt, c->liopCnt.p, 4, hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  c->liopCounters[0]++; c->liopCounters[1] += n; c->liopCounters[2] += (long)cnt; c->liopCounters[3] += subBatches;
  return MODSX_OK;
}

// ---- the normalised patches ----
static int tail_patches(modsx_ctx *c, void *self, const DescJob *jobs, int n, const float *grid, const int *needTab, const float *coordTab,
                        int photoNorm) {
  launch_describe_patch(c->stream, jobs, n, (const ImgRef *)c->imgRefs.p, grid, needTab, coordTab, c->dSiftMaskIdx, c->nSiftMask,
                        photoNorm, (float *)self, 1);
  return MODSX_OK;
}

int extract_patches(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                    int photoNorm, float *patches, bool onDevice) {
  if (patchSize != LIOP_SIDE) { set_error("modsx_extract_patches: patchSize must be 41"); return MODSX_ERR_ARG; }
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  const size_t bytes = (size_t)n * LIOP_PATCH_B;
  float *dst = patches;
  if (!onDevice) { if (!c->liopOut.ensure(bytes)) return MODSX_ERR_NOMEM; dst = (float *)c->liopOut.p; }
  const std::vector<modsx_region> v(regs, regs + n);
  const DescTail tail = {tail_patches, dst};
  int rc = describe_batch_tail(c, img, v, mrSize, patchSize, fast, photoNorm, tail);
  if (rc) return rc;
  if (!onDevice) MX_HIP(hipMemcpy(patches, dst, bytes, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

// ---- LIOP of patches ----
int liop_patches(modsx_ctx *c, const float *patches, int n, int patchSize, float *desc, bool onDevice, int *dbgPath, int *dbgPerm) {
  if (patchSize != LIOP_SIDE) { set_error("modsx_liop_patches: patchSize must be 41"); return MODSX_ERR_ARG; }
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  int rc = ensure_tables(c);
  if (rc) return rc;
  if ((rc = zero_counter(c))) return rc;
  const bool dbg = dbgPath || dbgPerm;
  int *dPath = nullptr, *dPerm = nullptr;
  if (dbg) {
    if (!c->liopDbg.ensure((size_t)n * (1 + LIOP_N) * 4)) return MODSX_ERR_NOMEM;
    dPath = (int *)c->liopDbg.p; dPerm = dPath + n;
  }
  long subBatches = 0;
  if (onDevice) {
    // rows that already live in HBM are read where they are
    launch_liop(c->stream, patches, n, desc, nullptr, tab_pixels(c), tab_samples(c), (unsigned *)c->liopCnt.p, dPath, dPerm);
    subBatches = 1;
  } else {
    const int B = std::min(liop_batch(), n);
    if (!c->liopPatches.ensure((size_t)B * LIOP_PATCH_B) || !c->liopOut.ensure((size_t)n * LIOP_DIM * 4)) return MODSX_ERR_NOMEM;
    for (int j0 = 0; j0 < n; j0 += B, subBatches++) {
      const int nb = std::min(B, n - j0);
      MX_HIP(hipMemcpyAsync(c->liopPatches.p, patches + (size_t)j0 * LIOP_NPX, (size_t)nb * LIOP_PATCH_B, hipMemcpyHostToDevice, c->stream));
      launch_liop(c->stream, (const float *)c->liopPatches.p, nb, (float *)c->liopOut.p + (size_t)j0 * LIOP_DIM, nullptr, tab_pixels(c),
                  tab_samples(c), (unsigned *)c->liopCnt.p, dPath ? dPath + j0 : nullptr, dPerm ? dPerm + (size_t)j0 * LIOP_N : nullptr);
    }
  }
  if ((rc = book_call(c, n, subBatches))) return rc;
  if (!onDevice) MX_HIP(hipMemcpy(desc, c->liopOut.p, (size_t)n * LIOP_DIM * 4, hipMemcpyDeviceToHost));
  if (dbgPath) MX_HIP(hipMemcpy(dbgPath, dPath, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (dbgPerm) MX_HIP(hipMemcpy(dbgPerm, dPerm, (size_t)n * LIOP_N * 4, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

// ---- regions -> LIOP ----
struct LiopTail { float *out; long subBatches; };
static int tail_liop(modsx_ctx *c, void *self, const DescJob *jobs, int n, const float *grid, const int *needTab, const float *coordTab,
                     int photoNorm) {
  LiopTail *lt = (LiopTail *)self;
  const int B = std::min(liop_batch(), n);
  if (!c->liopPatches.ensure((size_t)B * LIOP_PATCH_B)) return MODSX_ERR_NOMEM;
  // the launches of a stream run in order: sub-batch k + 1 overwrites the buffer after k_liop of sub-batch k has read it
  for (int j0 = 0; j0 < n; j0 += B, lt->subBatches++) {
    const int nb = std::min(B, n - j0);
    launch_describe_patch(c->stream, jobs + j0, nb, (const ImgRef *)c->imgRefs.p, grid, needTab, coordTab, c->dSiftMaskIdx, c->nSiftMask,
                          photoNorm, (float *)c->liopPatches.p, 0);
    launch_liop(c->stream, (const float *)c->liopPatches.p, nb, lt->out, jobs + j0, tab_pixels(c), tab_samples(c),
                (unsigned *)c->liopCnt.p, nullptr, nullptr);
  }
  return MODSX_OK;
}

int describe_regions_liop(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                          int photoNorm, float *desc, bool onDevice) {
  if (patchSize != LIOP_SIDE) { set_error("modsx_describe_regions_liop: patchSize must be 41"); return MODSX_ERR_ARG; }
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  int rc = ensure_tables(c);
  if (rc) return rc;
  if ((rc = zero_counter(c))) return rc;
  const size_t bytes = (size_t)n * LIOP_DIM * 4;
  LiopTail lt = {desc, 0};
  if (!onDevice) { if (!c->liopOut.ensure(bytes)) return MODSX_ERR_NOMEM; lt.out = (float *)c->liopOut.p; }
  const std::vector<modsx_region> v(regs, regs + n);
  const DescTail tail = {tail_liop, &lt};
  rc = describe_batch_tail(c, img, v, mrSize, patchSize, fast, photoNorm, tail);
  if (rc) return rc;
  if ((rc = book_call(c, n, lt.subBatches))) return rc;
  if (!onDevice) MX_HIP(hipMemcpy(desc, lt.out, bytes, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

}  // namespace mx
