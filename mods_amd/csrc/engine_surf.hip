// engine_surf.hip -- DescribeRegions<SURFDescriptor> (synth-detection.hpp:169-255 with descriptors/surfdescriptor.hpp:13-37,
// called at imagerepresentation.cpp:1829-1838): OpenSURF's upright SURF-64 of one fixed point on the normalised 41 x 41 patch.
//   * the functor's point (x = y = patchSize / 2.0f, scale = (float)(patchSize / mrSize)) makes every sample coordinate and
//     every gaussian weight of Surf::getDescriptor(true) a constant of (patchSize, mrSize): surf_tables builds them on the host
//     with the reference's f32 / f64 expressions and libm's expf (the overload the reference's object imports); the device copy
//     is cached per context and per mrSize;
//   * patches take the route of every patch descriptor (engine_patchdesc.hip): caller-supplied rows, or the description front
//     end with the patch-out form of k_describe, in sub-batches (MODSX_SURF_BATCH = patches per sub-batch), each followed by k_surf.
// mrSize is used twice, as the reference uses it: for the measurement window and for the scale of the point.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>
#include "engine_api.hpp"

namespace mx {

constexpr int SURF_SIDE = 41, SURF_DIM = MODSX_SURF_DIM;
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

static void run_surf(void *self, hipStream_t s, const float *patches, int nb, int first, float *out, const DescJob *jobs) {
  launch_surf(s, patches, nb, out, jobs, (const SurfTab *)self);
}
static PatchDesc surf_desc(const SurfTab *tab) { return {SURF_DIM, "MODSX_SURF_BATCH", run_surf, (void *)tab}; }

static int finish(modsx_ctx *c, int n, long subBatches, float *desc, bool onDevice) {
  const int rc = patch_sync(c);
  if (rc) return rc;
  c->surfCounters[0]++; c->surfCounters[1] += n; c->surfCounters[2] += subBatches;
  return patch_fetch(c, desc, (size_t)n * SURF_DIM, onDevice);
}

// ---- SURF of patches ----
int surf_patches(modsx_ctx *c, const float *patches, int n, double mrSize, float *desc, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  const SurfTab *tab = nullptr;
  int rc = ensure_table(c, mrSize, &tab);
  if (rc) return rc;
  long subBatches = 0;
  if ((rc = patchdesc_patches(c, surf_desc(tab), patches, n, desc, onDevice, &subBatches))) return rc;
  return finish(c, n, subBatches, desc, onDevice);
}

// ---- regions -> SURF ----
int describe_regions_surf(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                          int photoNorm, float *desc, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  const SurfTab *tab = nullptr;
  int rc = ensure_table(c, mrSize, &tab);
  if (rc) return rc;
  long subBatches = 0;
  if ((rc = patchdesc_regions(c, surf_desc(tab), img, regs, n, mrSize, patchSize, fast, photoNorm, desc, onDevice, &subBatches))) return rc;
  return finish(c, n, subBatches, desc, onDevice);
}

}  // namespace mx
