// engine_daisy.hip -- DescribeRegions<DAISYDescriptor> (synth-detection.hpp:169-255 with descriptors/daisydescriptor.hpp:33-92,
// called at imagerepresentation.cpp:1954-1963): libdaisy's descriptor of one fixed point on the normalised 41 x 41 patch.
//   * the functor's point (x = y = patchSize / 2, orientation 0) and set_parameters(rad, radq, thq, histq) make the filters, the
//     layer directions, the grid points and their bilinear weights constants of (rad, radq, thq): daisy_tables builds them on the
//     host with the reference's f32 / f64 expressions and libm's expf, cos and sin (the reference's object imports expf and
//     sincos); the device copy is cached per context and per triple;
//   * patches take the route of every patch descriptor (engine_patchdesc.hip): caller-supplied rows, or the description front
//     end with the patch-out form of k_describe, in sub-batches (MODSX_DAISY_BATCH = patches per sub-batch), each followed by k_daisy.
// mrSize only sizes the measurement window: the DAISY point and its grid do not depend on it.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <algorithm>
#include <string>
#include "engine_api.hpp"

namespace mx {

constexpr int DAISY_SIDE = 41, DAISY_HISTQ = 8;
enum { DAISY_SKIPPED = 0, DAISY_ZEROED = 1, DAISY_SAMPLED = 2 };

int daisy_check_args(const char *fn, int patchSize, int rad, int radq, int thq, int histq, int nrmType) {
  const char *what = nullptr;
  if (patchSize != DAISY_SIDE) what = "patchSize must be 41";
  else if (histq != DAISY_HISTQ) what = "histq must be 8";
  else if (thq < 1 || thq > 8) what = "thq must be 1 .. 8";
  else if (radq < 1 || radq > 3) what = "radq must be 1 .. 3";
  else if (rad < 1 || rad > 20) what = "rad must be 1 .. 20";
  else if (nrmType < 0 || nrmType > 2) what = "nrm_type must be 0 (partial), 1 (full) or 2 (sift)";
  if (!what) return MODSX_OK;
  set_error(std::string(fn) + ": " + what);
  return MODSX_ERR_ARG;
}

int daisy_dim(int radq, int thq, int histq) {
  if (daisy_check_args("modsx_daisy_dim", DAISY_SIDE, 1, radq, thq, histq, 0)) return MODSX_ERR_ARG;
  return (radq * thq + 1) * histq;
}

// daisy::filter_size, daisy.cpp:605-616
static int filter_size(double sigma) {
  int fsz = (int)(5 * sigma);
  if (fsz % 2 == 0) fsz++;
  if (fsz < 3) fsz = 3;
  return fsz;
}
// kutility::gaussian_1d(fltr, fsz, sigma, 0), math.hpp:29-48; the reference's object calls expf
static void gaussian_1d(float *fltr, int fsz, float sigma) {
  const int sz = (fsz - 1) / 2;
  const float mean = 0.0f, v = 2 * sigma * sigma;
  float sum = 0.0f;
  int counter = -1;
  for (int x = -sz; x <= sz; x++) {
    counter++;
    fltr[counter] = expf((-(x - mean) * (x - mean)) / v);
    sum += fltr[counter];
  }
  if (sum != 0)
    for (int x = 0; x < fsz; x++) fltr[x] /= sum;
}

static void fill_tab(int rad, int radq, int thq, DaisyTab *t, int *selected) {
  const float m_rad = (float)rad;          // daisy::m_rad is a float
  const double PI = 3.141592653589793;     // kutility_def.hpp
  *t = DaisyTab{};
  t->npts = radq * thq + 1;
  t->nfilt = 1 + radq;
  t->dim = t->npts * DAISY_HISTQ;
  gaussian_1d(t->k5, 5, 0.5f);
  // layered_gradient, math.hpp:773-777: pi() is atan2 of floats returned as float, cos and sin are the double ones
  const float pif = atan2f(0.0f, -1.0f);
  for (int l = 0; l < DAISY_HISTQ; l++) {
    const float angle = 2 * l * pif / DAISY_HISTQ;
    t->kos[l] = (float)cos((double)angle);
    t->zin[l] = (float)sin((double)angle);
  }
  // compute_cube_sigmas; smooth_layers' sigma is a float parameter, the incremental ones stay double
  double cs[3];
  const double r_step_d = double(m_rad) / radq;
  for (int r = 0; r < radq; r++) cs[r] = (r + 1) * r_step_d / 2;
  double sig[4];
  sig[0] = (double)(float)sqrt(1.6 * 1.6 - 0.25);
  for (int r = 0; r < radq; r++) sig[1 + r] = r == 0 ? cs[0] : sqrt(cs[r] * cs[r] - cs[r - 1] * cs[r - 1]);
  for (int f = 0; f < t->nfilt; f++) {
    t->fsz[f] = filter_size(sig[f]);
    gaussian_1d(t->taps + f * DAISY_TAP_ROW + DAISY_TAP_PAD, t->fsz[f], (float)sig[f]);
  }
  // update_selected_cubes, quantize_radius(float)
  int sel[3] = {0, 0, 0};
  for (int r = 0; r < radq; r++) {
    const double seed_sigma = (r + 1) * m_rad / radq / 2.0;
    const float q = (float)seed_sigma;
    if (q <= cs[0]) sel[r] = 0;
    else if (q >= cs[radq - 1]) sel[r] = radq - 1;
    else {
      float mindist = FLT_MAX;
      for (int c = 0; c < radq; c++) {
        const float dist = (float)fabs(cs[c] - q);
        if (dist < mindist) { mindist = dist; sel[r] = c; }
      }
    }
    if (selected) selected[r] = sel[r];
  }
  // compute_grid_points (r_step is a float quotient widened), compute_oriented_grid_points at orientation 0, then the point of
  // get_descriptor(20, 20, 0): i_get_descriptor's skip, bi_get_histogram's zero fill and weights
  const double r_step = m_rad / radq, t_step = 2 * PI / thq;
  const double angle0 = -0 * 2.0 * PI / 360, kos0 = cos(angle0), zin0 = sin(angle0);
  const double cy = DAISY_SIDE / 2, cx = DAISY_SIDE / 2;
  for (int g = 0; g < t->npts; g++) {
    double gy = 0, gx = 0;
    const int r = g == 0 ? 0 : (g - 1) / thq, th = g == 0 ? 0 : (g - 1) % thq;
    if (g > 0) {
      const double pr = (r + 1) * r_step, pt = th * t_step;
      const double x = pr * cos(pt), y = pr * sin(pt);
      gx = x * kos0 + y * zin0;
      gy = -x * zin0 + y * kos0;
    }
    t->cube[g] = sel[r];
    const double yy = cy + gy, xx = cx + gx;
    const bool outside = !(xx >= 0 && xx < DAISY_SIDE - 1) || !(yy >= 0 && yy < DAISY_SIDE - 1);
    if (g > 0 && outside) { t->state[g] = DAISY_SKIPPED; continue; }
    const int mnx = int(xx), mny = int(yy);
    if (mnx >= DAISY_SIDE - 2 || mny >= DAISY_SIDE - 2) { t->state[g] = DAISY_ZEROED; continue; }
    const double alpha = mnx + 1 - xx, beta = mny + 1 - yy;
    const float w0 = alpha * beta;
    const float w1 = beta - w0;
    const float w2 = alpha - w0;
    const float w3 = 1 + w0 - alpha - beta;
    t->state[g] = DAISY_SAMPLED;
    t->base[g] = mny * DAISY_SIDE + mnx;
    t->w[4 * g] = w0; t->w[4 * g + 1] = w1; t->w[4 * g + 2] = w2; t->w[4 * g + 3] = w3;
  }
}

int daisy_tables(int rad, int radq, int thq, int histq, float *k5, float *kos8, float *zin8, int *fsz, float *taps, int *selected,
                 int *state, int *base, float *w) {
  const int rc = daisy_check_args("modsx_daisy_tables", DAISY_SIDE, rad, radq, thq, histq, 0);
  if (rc) return rc;
  DaisyTab t;
  int sel[3];
  fill_tab(rad, radq, thq, &t, sel);
  if (k5) std::copy(t.k5, t.k5 + 5, k5);
  if (kos8) std::copy(t.kos, t.kos + 8, kos8);
  if (zin8) std::copy(t.zin, t.zin + 8, zin8);
  if (fsz) std::copy(t.fsz, t.fsz + t.nfilt, fsz);
  if (taps)
    for (int f = 0; f < t.nfilt; f++) {
      const float *row = t.taps + f * DAISY_TAP_ROW + DAISY_TAP_PAD;
      std::copy(row, row + DAISY_MAX_TAPS, taps + f * DAISY_MAX_TAPS);
    }
  if (selected) std::copy(sel, sel + radq, selected);
  if (state) std::copy(t.state, t.state + t.npts, state);
  if (base) std::copy(t.base, t.base + t.npts, base);
  if (w) std::copy(t.w, t.w + 4 * t.npts, w);
  return MODSX_OK;
}

// the device table of a triple: a slot that holds it, or the next slot round robin.  Calls on a context are synchronous, so no
// launch is reading the slot that is refilled
static int ensure_table(modsx_ctx *c, int rad, int radq, int thq, const DaisyTab **out) {
  const int key = rad << 16 | radq << 8 | thq;
  for (int i = 0; i < modsx_ctx::DAISY_TABS; i++)
    if (c->daisyTabKey[i] == key && c->daisyTab[i].p) { *out = (const DaisyTab *)c->daisyTab[i].p; return MODSX_OK; }
  DaisyTab t;
  fill_tab(rad, radq, thq, &t, nullptr);
  const int slot = c->daisyTabNext;
  c->daisyTabKey[slot] = 0;
  if (!c->daisyTab[slot].ensure(sizeof(DaisyTab))) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemcpy(c->daisyTab[slot].p, &t, sizeof(DaisyTab), hipMemcpyHostToDevice));
  c->daisyTabKey[slot] = key;
  c->daisyTabNext = (slot + 1) % modsx_ctx::DAISY_TABS;
  *out = (const DaisyTab *)c->daisyTab[slot].p;
  return MODSX_OK;
}

struct DaisyRun { const DaisyTab *tab; int nrmType; };
static void run_daisy(void *self, hipStream_t s, const float *patches, int nb, int first, float *out, const DescJob *jobs) {
  const DaisyRun *r = (const DaisyRun *)self;
  launch_daisy(s, patches, nb, out, jobs, r->tab, r->nrmType);
}
static PatchDesc daisy_desc(DaisyRun *r, int radq, int thq) { return {(radq * thq + 1) * DAISY_HISTQ, "MODSX_DAISY_BATCH", run_daisy, r}; }

static int finish(modsx_ctx *c, const PatchDesc &d, int n, long subBatches, float *desc, bool onDevice) {
  const int rc = patch_sync(c);
  if (rc) return rc;
  c->daisyCounters[0]++; c->daisyCounters[1] += n; c->daisyCounters[2] += subBatches;
  return patch_fetch(c, desc, (size_t)n * d.dim, onDevice);
}

// ---- DAISY of patches ----
int daisy_patches(modsx_ctx *c, const float *patches, int n, int rad, int radq, int thq, int nrmType, float *desc, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  DaisyRun r = {nullptr, nrmType};
  int rc = ensure_table(c, rad, radq, thq, &r.tab);
  if (rc) return rc;
  const PatchDesc d = daisy_desc(&r, radq, thq);
  long subBatches = 0;
  if ((rc = patchdesc_patches(c, d, patches, n, desc, onDevice, &subBatches))) return rc;
  return finish(c, d, n, subBatches, desc, onDevice);
}

// ---- regions -> DAISY ----
int describe_regions_daisy(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                           int photoNorm, int rad, int radq, int thq, int nrmType, float *desc, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  DaisyRun r = {nullptr, nrmType};
  int rc = ensure_table(c, rad, radq, thq, &r.tab);
  if (rc) return rc;
  const PatchDesc d = daisy_desc(&r, radq, thq);
  long subBatches = 0;
  if ((rc = patchdesc_regions(c, d, img, regs, n, mrSize, patchSize, fast, photoNorm, desc, onDevice, &subBatches))) return rc;
  return finish(c, d, n, subBatches, desc, onDevice);
}

}  // namespace mx
