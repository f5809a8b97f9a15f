// engine_surf.hip -- DescribeRegions<SURFDescriptor> (synth-detection.hpp:169-255 with descriptors/surfdescriptor.hpp:13-37,
// called at imagerepresentation.cpp:1829-1838): OpenSURF's upright SURF-64 of one fixed point on the normalised 41 x 41 patch.
//   * the functor's point (x = y = patchSize / 2.0f, scale = (float)(patchSize / mrSize)) makes every sample coordinate and
//     every gaussian weight of Surf::getDescriptor(true) a constant of (patchSize, mrSize): surf_tables builds them on the host
//     with the reference's f32 / f64 expressions and libm's expf (the overload the reference's object imports); the device copy
//     is cached per context and per mrSize;
//   * patches come from the description front end unchanged, as for LIOP (engine_liop.hip): the patch-out form of k_describe
//     as the last launch of a chunk, through the context's patch buffer of at most 64 MiB in sub-batches (MODSX_SURF_BATCH =
//     patches per sub-batch, read once per process), each followed by k_surf.
// mrSize is used twice, as the reference uses it: for the measurement window and for the scale of the point.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

constexpr int SURF_SIDE = 41, SURF_NPX = SURF_SIDE * SURF_SIDE, SURF_DIM = MODSX_SURF_DIM;
constexpr size_t SURF_PATCH_B = (size_t)SURF_NPX * 4, SURF_BUF_B = (size_t)64 << 20;
constexpr double SURF_MAX_SCALE = 1024.0;      // modsx.h: patchSize / mrSize above this is refused

// fRound, opensurf/utils.h:58-61
static int f_round(float flt) { return (int)floorf(flt + 0.5f); }
// Surf::gaussian(int, int, float) and (float, float, float), opensurf/surf.cpp:253-265, pi = 3.14159f; the reference's object
// calls expf for both
static const float SURF_PI = 3.14159f;
static float gaussian_i(int x, int y, float sig) { return (1.0f / (2.0f * SURF_PI * sig * sig)) * expf(-(x * x + y * y) / (2.0f * sig * sig)); }
static float gaussian_f(float x, float y, float sig) { return 1.0f / (2.0f * SURF_PI * sig * sig) * expf(-(x * x + y * y) / (2.0f * sig * sig)); }

int surf_check_args(const char *fn, int patchSize, double mrSize) {
  if (patchSize != SURF_SIDE) { set_error(std::string(fn) + ": patchSize must be 41"); return MODSX_ERR_ARG; }
  if (!std::isfinite(mrSize) || !(mrSize > 0.0) || (double)(float)patchSize / mrSize > SURF_MAX_SCALE) {
    set_error(std::string(fn) + ": mrSize must be finite, positive and at least patchSize / 1024");
    return MODSX_ERR_ARG;
  }
  return MODSX_OK;
}

// the loops of Surf::getDescriptor(true) (surf.cpp:152-240) without the image: i, j in {-12, -7, -2, 3}, k in [i, i + 9),
// l in [j, j + 9).  sample_x depends on k alone and sample_y on l alone (si = 0: the -l*scale*si term is a zero of either sign)
int surf_tables(int patchSize, double mrSize, int *sample_x24, int *sample_y24, float *w1, float *w2, int *haar_size) {
  const int rc = surf_check_args("modsx_surf_tables", patchSize, mrSize);
  if (rc) return rc;
  const float scale = float(patchSize) / mrSize;
  const int x = f_round((float)patchSize / 2.0f), y = f_round((float)patchSize / 2.0f);
  const float co = 1, si = 0;
  float cx = -0.5f, cy = 0.f;
  int q = 0;
  for (int i = -12; i < 8; i += 5) {
    cx += 1.f;
    cy = -0.5f;
    for (int j = -12; j < 8; j += 5, q++) {
      cy += 1.f;
      const int ix = i + 5, jx = j + 5;
      const int xs = f_round(x + (-jx * scale * si + ix * scale * co));
      const int ys = f_round(y + (jx * scale * co + ix * scale * si));
      int t = 0;
      for (int k = i; k < i + 9; ++k)
        for (int l = j; l < j + 9; ++l, ++t) {
          const int sample_x = f_round(x + (-l * scale * si + k * scale * co));
          const int sample_y = f_round(y + (l * scale * co + k * scale * si));
          if (sample_x24) sample_x24[k + 12] = sample_x;
          if (sample_y24) sample_y24[l + 12] = sample_y;
          if (w1) w1[q * 81 + t] = gaussian_i(xs - sample_x, ys - sample_y, 2.5f * scale);
        }
      if (w2) w2[q] = gaussian_f(cx - 2.0f, cy - 2.0f, 1.5f);
    }
  }
  if (haar_size) *haar_size = 2 * f_round(scale);
  return MODSX_OK;
}

// the device table of mrSize: a slot that holds it, or the next slot round robin.  Calls on a context are synchronous, so no
// launch is reading the slot that is refilled
static int ensure_table(modsx_ctx *c, double mrSize, const SurfTab **out) {
  for (int i = 0; i < modsx_ctx::SURF_TABS; i++)
    if (c->surfTabMr[i] == mrSize && c->surfTab[i].p) { *out = (const SurfTab *)c->surfTab[i].p; return MODSX_OK; }
  SurfTab t = {};
  int rc = surf_tables(SURF_SIDE, mrSize, t.sx, t.sy, t.w1, t.w2, &t.haar);
  if (rc) return rc;
  const int slot = c->surfTabNext;
  c->surfTabMr[slot] = 0;
  if (!c->surfTab[slot].ensure(sizeof(SurfTab))) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemcpy(c->surfTab[slot].p, &t, sizeof(SurfTab), hipMemcpyHostToDevice));
  c->surfTabMr[slot] = mrSize;
  c->surfTabNext = (slot + 1) % modsx_ctx::SURF_TABS;
  *out = (const SurfTab *)c->surfTab[slot].p;
  return MODSX_OK;
}

// patches per sub-batch: what fits 64 MiB, or MODSX_SURF_BATCH (1 .. that many), read once per process
static int surf_batch() {
  static const int b = [] {
    const long full = (long)(SURF_BUF_B / SURF_PATCH_B);
    const char *e = getenv("MODSX_SURF_BATCH");
    const long v = e ? atol(e) : full;
    return (int)std::min(std::max(v, 1L), full);
  }();
  return b;
}

static int book_call(modsx_ctx *c, int n, long subBatches) {
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  c->surfCounters[0]++; c->surfCounters[1] += n; c->surfCounters[2] += subBatches;
  return MODSX_OK;
}

// ---- SURF of patches ----
int surf_patches(modsx_ctx *c, const float *patches, int n, double mrSize, float *desc, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  const SurfTab *tab = nullptr;
  int rc = ensure_table(c, mrSize, &tab);
  if (rc) return rc;
  long subBatches = 0;
  if (onDevice) {
    // rows that already live in HBM are read where they are
    launch_surf(c->stream, patches, n, desc, nullptr, tab);
    subBatches = 1;
  } else {
    const int B = std::min(surf_batch(), n);
    if (!c->liopPatches.ensure((size_t)B * SURF_PATCH_B) || !c->surfOut.ensure((size_t)n * SURF_DIM * 4)) return MODSX_ERR_NOMEM;
    for (int j0 = 0; j0 < n; j0 += B, subBatches++) {
      const int nb = std::min(B, n - j0);
      MX_HIP(hipMemcpyAsync(c->liopPatches.p, patches + (size_t)j0 * SURF_NPX, (size_t)nb * SURF_PATCH_B, hipMemcpyHostToDevice, c->stream));
      launch_surf(c->stream, (const float *)c->liopPatches.p, nb, (float *)c->surfOut.p + (size_t)j0 * SURF_DIM, nullptr, tab);
    }
  }
  if ((rc = book_call(c, n, subBatches))) return rc;
  if (!onDevice) MX_HIP(hipMemcpy(desc, c->surfOut.p, (size_t)n * SURF_DIM * 4, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

// ---- regions -> SURF ----
struct SurfTail { float *out; const SurfTab *tab; long subBatches; };
static int tail_surf(modsx_ctx *c, void *self, const DescJob *jobs, int n, const float *grid, const int *needTab, const float *coordTab,
                     int photoNorm) {
  SurfTail *st = (SurfTail *)self;
  const int B = std::min(surf_batch(), n);
  if (!c->liopPatches.ensure((size_t)B * SURF_PATCH_B)) return MODSX_ERR_NOMEM;
  // the launches of a stream run in order: sub-batch k + 1 overwrites the buffer after k_surf of sub-batch k has read it
  for (int j0 = 0; j0 < n; j0 += B, st->subBatches++) {
    const int nb = std::min(B, n - j0);
    launch_describe_patch(c->stream, jobs + j0, nb, (const ImgRef *)c->imgRefs.p, grid, needTab, coordTab, c->dSiftMaskIdx, c->nSiftMask,
                          photoNorm, (float *)c->liopPatches.p, 0);
    launch_surf(c->stream, (const float *)c->liopPatches.p, nb, st->out, jobs + j0, st->tab);
  }
  return MODSX_OK;
}

int describe_regions_surf(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                          int photoNorm, float *desc, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  SurfTail st = {desc, nullptr, 0};
  int rc = ensure_table(c, mrSize, &st.tab);
  if (rc) return rc;
  const size_t bytes = (size_t)n * SURF_DIM * 4;
  if (!onDevice) { if (!c->surfOut.ensure(bytes)) return MODSX_ERR_NOMEM; st.out = (float *)c->surfOut.p; }
  const std::vector<modsx_region> v(regs, regs + n);
  const DescTail tail = {tail_surf, &st};
  rc = describe_batch_tail(c, img, v, mrSize, patchSize, fast, photoNorm, tail);
  if (rc) return rc;
  if ((rc = book_call(c, n, st.subBatches))) return rc;
  if (!onDevice) MX_HIP(hipMemcpy(desc, st.out, bytes, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

}  // namespace mx
