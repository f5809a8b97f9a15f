// engine_liop.hip -- DescribeRegions<LIOPDescriptor> (synth-detection.hpp:169-255 with matching/liopdesc.hpp:55-63) and the
// normalised patches DescribeRegions<> hands to any functor, as device outputs.
//   * the tables of vl_liopdesc_new_basic(41) (vlfeat/vl/liop.c:346-395) are built here on the host, with libm as the reference
//     builds them, once per context;
//   * patches come from the description front end unchanged: the windows, the chunk planner (describe_plan.cpp) and the sampling
//     and blur launches of describe_batch, with the patch-out form of k_describe as the last launch (DescTail);
//   * a LIOP call takes the route of every patch descriptor (engine_patchdesc.hip): sub-batches of caller-supplied rows or of a
//     chunk's jobs, patch-out launch then k_liop (MODSX_LIOP_BATCH = patches per sub-batch).
// LIOP has no parameters of its own: the ini's neighbours / bins / radius / threshold keys never reach VLFeat.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

constexpr int LIOP_SIDE = 41, LIOP_NPX = LIOP_SIDE * LIOP_SIDE, LIOP_N = MODSX_LIOP_PIXELS, LIOP_DIM = MODSX_LIOP_DIM;
constexpr size_t LIOP_PATCH_B = (size_t)LIOP_NPX * 4;
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

static int zero_counter(modsx_ctx *c) {
  if (!c->liopCnt.ensure(16)) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemsetAsync(c->liopCnt.p, 0, 16, c->stream));
  return MODSX_OK;
}
// the exact-path counter rides the call's one wait; then the call is booked and a host caller gets its rows
static int finish(modsx_ctx *c, int n, long subBatches, float *desc, bool onDevice) {
  unsigned cnt = 0;
  MX_HIP(hipMemcpyAsync(&cnt, c->liopCnt.p, 4, hipMemcpyDeviceToHost, c->stream));
  const int rc = patch_sync(c);
  if (rc) return rc;
  c->liopCounters[0]++; c->liopCounters[1] += n; c->liopCounters[2] += (long)cnt; c->liopCounters[3] += subBatches;
  return patch_fetch(c, desc, (size_t)n * LIOP_DIM, onDevice);
}

struct LiopRun { const unsigned short *pixels; const LiopSample *samples; unsigned *cnt; int *dPath, *dPerm; };
static void run_liop(void *self, hipStream_t s, const float *patches, int nb, int first, float *out, const DescJob *jobs) {
  const LiopRun *r = (const LiopRun *)self;
  launch_liop(s, patches, nb, out, jobs, r->pixels, r->samples, r->cnt, r->dPath ? r->dPath + first : nullptr,
              r->dPerm ? r->dPerm + (size_t)first * LIOP_N : nullptr);
}
// the tables and a zeroed exact-path counter on the device: what every LIOP call starts with
static int liop_begin(modsx_ctx *c, LiopRun *r) {
  int rc = ensure_tables(c);
  if (rc) return rc;
  if ((rc = zero_counter(c))) return rc;
  *r = {tab_pixels(c), tab_samples(c), (unsigned *)c->liopCnt.p, nullptr, nullptr};
  return MODSX_OK;
}
static PatchDesc liop_desc(LiopRun *r) { return {LIOP_DIM, "MODSX_LIOP_BATCH", run_liop, r}; }

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
  if (!onDevice) { if (!c->patchOut.ensure(bytes)) return MODSX_ERR_NOMEM; dst = (float *)c->patchOut.p; }
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
  LiopRun r;
  int rc = liop_begin(c, &r);
  if (rc) return rc;
  if (dbgPath || dbgPerm) {
    if (!c->liopDbg.ensure((size_t)n * (1 + LIOP_N) * 4)) return MODSX_ERR_NOMEM;
    r.dPath = (int *)c->liopDbg.p; r.dPerm = r.dPath + n;
  }
  long subBatches = 0;
  if ((rc = patchdesc_patches(c, liop_desc(&r), patches, n, desc, onDevice, &subBatches))) return rc;
  if ((rc = finish(c, n, subBatches, desc, onDevice))) return rc;
  if (dbgPath) MX_HIP(hipMemcpy(dbgPath, r.dPath, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (dbgPerm) MX_HIP(hipMemcpy(dbgPerm, r.dPerm, (size_t)n * LIOP_N * 4, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

// ---- regions -> LIOP ----
int describe_regions_liop(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                          int photoNorm, float *desc, bool onDevice) {
  if (patchSize != LIOP_SIDE) { set_error("modsx_describe_regions_liop: patchSize must be 41"); return MODSX_ERR_ARG; }
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  LiopRun r;
  int rc = liop_begin(c, &r);
  if (rc) return rc;
  long subBatches = 0;
  if ((rc = patchdesc_regions(c, liop_desc(&r), img, regs, n, mrSize, patchSize, fast, photoNorm, desc, onDevice, &subBatches))) return rc;
  return finish(c, n, subBatches, desc, onDevice);
}

}  // namespace mx
