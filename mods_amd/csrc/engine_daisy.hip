// engine_daisy.hip -- DescribeRegions<DAISYDescriptor> (synth-detection.hpp:169-255 with descriptors/daisydescriptor.hpp:33-92,
// called at imagerepresentation.cpp:1954-1963): libdaisy's descriptor of one fixed point on the normalised 41 x 41 patch.
//   * the functor's point (x = y = patchSize / 2, orientation 0) and set_parameters(rad, radq, thq, histq) make the filters, the
//     layer directions, the grid points and their bilinear weights constants of (rad, radq, thq): daisy_tables builds them on the
//     host with the reference's f32 / f64 expressions and libm's expf, cos and sin (the reference's object imports expf and
//     sincos); the device copy is cached per context and per triple;
//   * patches come from the description front end unchanged, as for LIOP and SURF: the patch-out form of k_describe as the last
//     launch of a chunk, through the context's patch buffer of at most 64 MiB in sub-batches (MODSX_DAISY_BATCH = patches per
//     sub-batch, read once per process), each followed by k_daisy.
// mrSize only sizes the measurement window: the DAISY point and its grid do not depend on it.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

constexpr int DAISY_SIDE = 41, DAISY_NPX = DAISY_SIDE * DAISY_SIDE, DAISY_HISTQ = 8;
constexpr size_t DAISY_PATCH_B = (size_t)DAISY_NPX * 4, DAISY_BUF_B = (size_t)64 << 20;
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

// patches per sub-batch: what fits 64 MiB, or MODSX_DAISY_BATCH (1 .. that many), read once per process
static int daisy_batch() {
  static const int b = [] {
    const long full = (long)(DAISY_BUF_B / DAISY_PATCH_B);
    const char *e = getenv("MODSX_DAISY_BATCH");
    const long v = e ? atol(e) : full;
    return (int)std::min(std::max(v, 1L), full);
  }();
  return b;
}

static int book_call(modsx_ctx *c, int n, long subBatches) {
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  c->daisyCounters[0]++; c->daisyCounters[1] += n; c->daisyCounters[2] += subBatches;
  return MODSX_OK;
}

// ---- DAISY of patches ----
int daisy_patches(modsx_ctx *c, const float *patches, int n, int rad, int radq, int thq, int nrmType, float *desc, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  const DaisyTab *tab = nullptr;
  int rc = ensure_table(c, rad, radq, thq, &tab);
  if (rc) return rc;
  const int dim = (radq * thq + 1) * DAISY_HISTQ;
  long subBatches = 0;
  if (onDevice) {
    // rows that already live in HBM are read where they are
    launch_daisy(c->stream, patches, n, desc, nullptr, tab, nrmType);
    subBatches = 1;
  } else {
    const int B = std::min(daisy_batch(), n);
    if (!c->liopPatches.ensure((size_t)B * DAISY_PATCH_B) || !c->daisyOut.ensure((size_t)n * dim * 4)) return MODSX_ERR_NOMEM;
    for (int j0 = 0; j0 < n; j0 += B, subBatches++) {
      const int nb = std::min(B, n - j0);
      MX_HIP(hipMemcpyAsync(c->liopPatches.p, patches + (size_t)j0 * DAISY_NPX, (size_t)nb * DAISY_PATCH_B, hipMemcpyHostToDevice, c->stream));
      launch_daisy(c->stream, (const float *)c->liopPatches.p, nb, (float *)c->daisyOut.p + (size_t)j0 * dim, nullptr, tab, nrmType);
    }
  }
  if ((rc = book_call(c, n, subBatches))) return rc;
  if (!onDevice) MX_HIP(hipMemcpy(desc, c->daisyOut.p, (size_t)n * dim * 4, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

// ---- regions -> DAISY ----
struct DaisyTail { float *out; const DaisyTab *tab; int nrmType; long subBatches; };
static int tail_daisy(modsx_ctx *c, void *self, const DescJob *jobs, int n, const float *grid, const int *needTab, const float *coordTab,
                      int photoNorm) {
  DaisyTail *dt = (DaisyTail *)self;
  const int B = std::min(daisy_batch(), n);
  if (!c->liopPatches.ensure((size_t)B * DAISY_PATCH_B)) return MODSX_ERR_NOMEM;
  // the launches of a stream run in order: sub-batch k + 1 overwrites the buffer after k_daisy of sub-batch k has read it
  for (int j0 = 0; j0 < n; j0 += B, dt->subBatches++) {
    const int nb = std::min(B, n - j0);
    launch_describe_patch(c->stream, jobs + j0, nb, (const ImgRef *)c->imgRefs.p, grid, needTab, coordTab, c->dSiftMaskIdx, c->nSiftMask,
                          photoNorm, (float *)c->liopPatches.p, 0);
    launch_daisy(c->stream, (const float *)c->liopPatches.p, nb, dt->out, jobs + j0, dt->tab, dt->nrmType);
  }
  return MODSX_OK;
}

int describe_regions_daisy(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                           int photoNorm, int rad, int radq, int thq, int nrmType, float *desc, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  DaisyTail dt = {desc, nullptr, nrmType, 0};
  int rc = ensure_table(c, rad, radq, thq, &dt.tab);
  if (rc) return rc;
  const size_t bytes = (size_t)n * (radq * thq + 1) * DAISY_HISTQ * 4;
  if (!onDevice) { if (!c->daisyOut.ensure(bytes)) return MODSX_ERR_NOMEM; dt.out = (float *)c->daisyOut.p; }
  const std::vector<modsx_region> v(regs, regs + n);
  const DescTail tail = {tail_daisy, &dt};
  rc = describe_batch_tail(c, img, v, mrSize, patchSize, fast, photoNorm, tail);
  if (rc) return rc;
  if ((rc = book_call(c, n, dt.subBatches))) return rc;
  if (!onDevice) MX_HIP(hipMemcpy(desc, dt.out, bytes, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

}  // namespace mx
