// capi.hip -- the extern "C" boundary declared in include/modsx.h.
#include <math.h>
#include <malloc.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include "batch_driver.hpp"
#include "engine_api.hpp"
#include "describe_plan.hpp"
#include "views_plan.hpp"
#include "describe_lanes.hpp"

using namespace mx;

#define NEED(c)                                             \
  do {                                                      \
    if (!(c)) { mx::set_error("null argument: " #c); return MODSX_ERR_ARG; } \
  } while (0)

// The host share of the process's last batch call (modsx_match_pairs, modsx_match_pairs_views, modsx_match_reps; for
// modsx_match_one_to_many the last round of its ladder): DuplicateFiltering + LO-RANSAC of its pairs are the tasks of run_batch
// (batch_driver.hpp), which resets these statistics when a run starts.
static mx::BatchStats g_batch;
// helper threads of a batch call: one per working context unless MODSX_VERIFY_HELPERS gives a smaller number
static int verify_helper_cap() {
  static const int cap = getenv("MODSX_VERIFY_HELPERS") ? atoi(getenv("MODSX_VERIFY_HELPERS")) : 0;
  return cap;
}

extern "C" {

int modsx_version(void) { return MODSX_VERSION; }
const char *modsx_last_error(void) { return mx::last_error(); }
void modsx_free(void *p) { free(p); }

// The host stages of a pair allocate and release ~100 MB of job tables, region lists and tentative arrays per call.  With
// glibc's defaults every block above 128 KB is its own mmap: fresh zero pages faulted in on first touch and unmapped on free --
// about 1 ms of page faults per 31-view pair (measured: 16.3 -> 15.3 ms).  Once per process the thresholds are raised so that
// such blocks come from, and return to, the heap and stay mapped.  This changes malloc for the whole host process, so it is
// OPT-IN: MODSX_MALLOC_TUNE=1 (bench.py and tools/latency.py set it; a host application decides for itself).
static void tune_host_allocator() {
#if defined(__GLIBC__)
  static std::once_flag once;
  std::call_once(once, [] {
    const char *e = getenv("MODSX_MALLOC_TUNE");
    if (!e || atoi(e) == 0) return;
    mallopt(M_MMAP_THRESHOLD, 1 << 30);
    mallopt(M_TRIM_THRESHOLD, 1 << 30);
    mallopt(M_TOP_PAD, 64 << 20);
  });
#endif
}

modsx_ctx *modsx_create(int device_id) {
  tune_host_allocator();
  return ctx_create(device_id);
}
void modsx_destroy(modsx_ctx *ctx) { ctx_destroy(ctx); }
int modsx_synchronize(modsx_ctx *ctx) {
  NEED(ctx);
  MX_HIP(hipStreamSynchronize(ctx->stream));
  return MODSX_OK;
}

void modsx_default_hessaff_params(modsx_hessaff_params *p) {
  // build/config_iter_mods_cviu.ini:13-27; structures.hpp:141-160; affine.h:47-58
  p->threshold = 5.3333f;
  p->mode = MODSX_FIXED_TH;
  p->reg_number = 2000;
  p->rel_threshold = -1;
  p->rel_reg_number = -1;
  p->numberOfScales = 3;
  p->initialSigma = 1.6f;
  p->edgeEigenValueRatio = 10.0;
  p->border = 5;
  p->maxIterations = 16;
  p->convergenceThreshold = 0.05f;
  p->smmWindowSize = 19;
  p->affInitialSigma = 1.6f;
  p->doBaumberg = 1;
  p->detectorType = MODSX_DET_HESSIAN;
}

void modsx_default_mser_params(modsx_mser_params *p);
void modsx_default_pair_params(modsx_pair_params *p) {
  memset(p, 0, sizeof *p);
  modsx_default_hessaff_params(&p->det);
  p->ori_mrSize = 1.0; p->ori_patchSize = 41; p->ori_maxAngles = 1; p->ori_threshold = 0.8;
  p->desc_mrSize = 5.1962; p->desc_patchSize = 41; p->desc_photoNorm = 1; p->desc_type = MODSX_DESC_ROOT_SIFT;
  p->desc_maxBinValue = 0.2;
  p->match_ratio = 0.8; p->contradDist = 30.0; p->nn = 50;
  p->duplicateDist = 2.0;
  p->err_threshold = 3.0; p->confidence = 0.99; p->max_samples = 100000; p->localOptimization = 1;
  p->HLAFCoef = 12.0; p->doSymmCheck = 1;
  p->ransac_seed = 1;
  p->useF = 0; p->LAFCoef = 2.0; p->errorType = 0;
  p->detector = MODSX_DET_HESSIAN;
  modsx_default_mser_params(&p->mser);
}

// the samplers address a pixel by a 24-bit row x column product and a 32-bit byte offset from the image base (kmath.hpp,
// bilinear_tap); views and pyramid levels are never larger than the image they come from by more than the rotation's
// bounding box (< 2x per side), so the bound is taken with that margin
static bool image_size_ok(int rows, int cols) {
  if (rows < 2 || cols < 2) {   // interpolate()'s clamp `min(max(x, 0), cols - 2)` needs two pixels per side (kmath.hpp bilinear_blend)
    mx::set_error("images of fewer than 2 rows or 2 columns are not supported");
    return false;
  }
  if (rows > 16384 || cols > 16384 || (long long)rows * cols > (1ll << 26)) {
    mx::set_error("image larger than 16384 px per side / 64 Mpx is not supported");
    return false;
  }
  return true;
}

modsx_image *modsx_image_upload(modsx_ctx *ctx, const void *pixels, int rows, int cols, int channels, int dtype) {
  if (!ctx || !pixels || rows <= 0 || cols <= 0 || (channels != 1 && channels != 3) || (dtype != 0 && dtype != 1)) {
    mx::set_error("modsx_image_upload: bad argument");
    return nullptr;
  }
  if (!image_size_ok(rows, cols)) return nullptr;
  hipSetDevice(ctx->dev);
  const size_t n = (size_t)rows * cols;
  const size_t inBytes = n * channels * (dtype == 0 ? 1 : 4);
  modsx_image *im = new modsx_image();
  im->rows = rows; im->cols = cols; im->owned = true; im->d = nullptr;
  if (hipMalloc(&im->d, n * 4) != hipSuccess) { mx::set_error("hipMalloc image"); delete im; return nullptr; }
  if (!ctx->misc.ensure(inBytes)) { hipFree(im->d); delete im; return nullptr; }
  if (hipMemcpyAsync(ctx->misc.p, pixels, inBytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
    mx::set_error("image H2D copy failed"); hipFree(im->d); delete im; return nullptr;
  }
  launch_gray(ctx->stream, ctx->misc.p, im->d, n, channels, dtype);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) { mx::set_error("image upload sync failed"); hipFree(im->d); delete im; return nullptr; }
  return im;
}

int modsx_image_update(modsx_ctx *ctx, modsx_image *im, const void *pixels, int rows, int cols, int channels, int dtype) {
  NEED(ctx); NEED(im); NEED(pixels);
  if ((channels != 1 && channels != 3) || (dtype != 0 && dtype != 1) || !im->owned || rows != im->rows || cols != im->cols) {
    mx::set_error("modsx_image_update: bad argument (the image must be an uploaded one of the same size)");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  const size_t n = (size_t)rows * cols, inBytes = n * channels * (dtype == 0 ? 1 : 4);
  if (!ctx->misc.ensure(inBytes)) return MODSX_ERR_NOMEM;
  if (hipMemcpyAsync(ctx->misc.p, pixels, inBytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { mx::set_error("image H2D copy failed"); return MODSX_ERR_DEVICE; }
  launch_gray(ctx->stream, ctx->misc.p, im->d, n, channels, dtype);
  // the caller's buffer is its own again on return (a copy from pageable memory is staged by the runtime; this wait also covers pinned sources)
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) { mx::set_error("image update sync failed"); return MODSX_ERR_DEVICE; }
  return MODSX_OK;
}

modsx_image *modsx_image_wrap_device(modsx_ctx *ctx, const float *dev_pixels, int rows, int cols) {
  if (!ctx || !dev_pixels || rows <= 0 || cols <= 0) { mx::set_error("modsx_image_wrap_device: bad argument"); return nullptr; }
  if (!image_size_ok(rows, cols)) return nullptr;
  modsx_image *im = new modsx_image();
  im->d = const_cast<float *>(dev_pixels); im->rows = rows; im->cols = cols; im->owned = false;
  return im;
}

void modsx_image_free(modsx_ctx *ctx, modsx_image *img) {
  if (!img) return;
  if (ctx) hipSetDevice(ctx->dev);
  if (img->owned && img->d) hipFree(img->d);
  delete img;
}

int modsx_image_download(modsx_ctx *ctx, const modsx_image *img, float *out) {
  NEED(ctx); NEED(img); NEED(out);
  MX_HIP(hipMemcpyAsync(out, img->d, (size_t)img->rows * img->cols * 4, hipMemcpyDeviceToHost, ctx->stream));
  MX_HIP(hipStreamSynchronize(ctx->stream));
  return MODSX_OK;
}

int modsx_detect_affine_keypoints(modsx_ctx *ctx, const modsx_image *img, const modsx_hessaff_params *par, double tilt,
                                  double zoom, modsx_keypoint **out) {
  NEED(ctx); NEED(img); NEED(par); NEED(out);
  hipSetDevice(ctx->dev);
  std::vector<modsx_keypoint> k[1];
  const modsx_image *imgs[1] = {img};
  int rc = detect_keypoints_batch(ctx, imgs, 1, *par, &tilt, &zoom, k);
  if (rc) return rc;
  *out = to_malloc(k[0]);
  return (int)k[0].size();
}

int modsx_detect_scalespace(modsx_ctx *ctx, const modsx_image *img, const modsx_hessaff_params *par, modsx_sskp **out) {
  NEED(ctx); NEED(img); NEED(par); NEED(out);
  hipSetDevice(ctx->dev);
  std::vector<modsx_sskp> k[1];
  const modsx_image *imgs[1] = {img};
  int rc = detect_scalespace_batch(ctx, imgs, 1, *par, k);
  if (rc) return rc;
  *out = to_malloc(k[0]);
  return (int)k[0].size();
}

int modsx_octave_levels(modsx_ctx *ctx, const modsx_image *img, const modsx_hessaff_params *par, float *blurs,
                        float *resps) {
  NEED(ctx); NEED(img); NEED(par); NEED(blurs); NEED(resps);
  hipSetDevice(ctx->dev);
  const modsx_image *imgs[1] = {img};
  int rc = build_pyramids(ctx, imgs, 1, *par, true);
  if (rc) return rc;
  const int L = par->numberOfScales + 2;
  const size_t npx = (size_t)img->rows * img->cols;
  const Octave &o = ctx->pyr[0].oct[0];
  for (int l = 0; l < L; l++) {
    MX_HIP(hipMemcpyAsync(blurs + l * npx, o.blur[l], npx * 4, hipMemcpyDeviceToHost, ctx->stream));
    MX_HIP(hipMemcpyAsync(resps + l * npx, o.resp[l], npx * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  MX_HIP(hipStreamSynchronize(ctx->stream));
  return L;
}

int modsx_gaussian_blur(modsx_ctx *ctx, const modsx_image *img, float sigma, float *out) {
  NEED(ctx); NEED(img); NEED(out);
  hipSetDevice(ctx->dev);
  const size_t npx = (size_t)img->rows * img->cols;
  if (!ctx->scratchA.ensure(npx * 4)) return MODSX_ERR_NOMEM;
  BlurBatch b;
  memset(&b, 0, sizeof b);
  int n = blur_ksize(sigma);
  if (n > MAX_TAPS) { mx::set_error("modsx_gaussian_blur: ksize > 17"); return MODSX_ERR_ARG; }
  if (n == 1) {
    MX_HIP(hipMemcpyAsync(out, img->d, npx * 4, hipMemcpyDeviceToHost, ctx->stream));
    MX_HIP(hipStreamSynchronize(ctx->stream));
    return MODSX_OK;
  }
  std::vector<float> k = gaussian_kernel(n, sigma);
  b.n = n;
  for (int i = 0; i < n; i++) b.k[i] = k[i];
  b.j[0].src = img->d; b.j[0].blur = (float *)ctx->scratchA.p; b.j[0].resp = nullptr; b.j[0].rows = img->rows;
  b.j[0].cols = img->cols; b.j[0].norm = 1.f;
  mx::book_blur(ctx, launch_blur_hess(ctx->stream, b, 1, img->rows, img->cols));
  MX_HIP(hipMemcpyAsync(out, ctx->scratchA.p, npx * 4, hipMemcpyDeviceToHost, ctx->stream));
  MX_HIP(hipStreamSynchronize(ctx->stream));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

// gaussianBlur(helpers.cpp:717-724) for any sigma (the tiled pyramid kernel stops at 17 taps): two generic passes, replicate border
static int blur_any(modsx_ctx *c, const float *src, float *dst, float *tmp, float *dTaps, float *hTaps, int rows, int cols, float sigma) {
  const int n = blur_ksize(sigma);
  if (n == 1) { MX_HIP(hipMemcpyAsync(dst, src, (size_t)rows * cols * 4, hipMemcpyDeviceToDevice, c->stream)); return MODSX_OK; }
  const int nx = cols == 1 ? 1 : n, ny = rows == 1 ? 1 : n;
  std::vector<float> kx = gaussian_kernel(nx, sigma), ky = gaussian_kernel(ny, sigma);
  memcpy(hTaps, kx.data(), nx * 4); memcpy(hTaps + nx, ky.data(), ny * 4);
  MX_HIP(hipMemcpyAsync(dTaps, hTaps, (size_t)(nx + ny) * 4, hipMemcpyHostToDevice, c->stream));
  launch_blur_pass(c->stream, src, tmp, rows, cols, dTaps, nx, 0, 1);
  launch_blur_pass(c->stream, tmp, dst, rows, cols, dTaps + nx, ny, 1, 1);
  return MODSX_OK;
}

int modsx_response(modsx_ctx *ctx, const modsx_image *img, int detector_type, float norm, float *out) {
  NEED(ctx); NEED(img); NEED(out);
  if (detector_type != MODSX_DET_HESSIAN && detector_type != MODSX_DET_DOG && detector_type != MODSX_DET_HARRIS) {
    mx::set_error("modsx_response: detector type must be Hessian (0), DoG (1) or Harris (2)");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  hipStream_t s = ctx->stream;
  const int rows = img->rows, cols = img->cols;
  const size_t npx = (size_t)rows * cols;
  const float sigma = detector_type == MODSX_DET_DOG ? norm : sqrtf((float)(0.6 * norm));
  const int ntap = 2 * std::max(1, blur_ksize(sigma)) * 3 + 16;
  if (ntap > 3 * 4096) { mx::set_error("modsx_response: blur kernel too large"); return MODSX_ERR_ARG; }
  if (!ctx->scratchA.ensure(npx * 4 * 8) || !ctx->viewTaps.ensure((size_t)ntap * 4) || !ctx->hViewTaps.ensure((size_t)ntap * 4)) return MODSX_ERR_NOMEM;
  float *buf = (float *)ctx->scratchA.p, *res = buf, *tmp = buf + npx, *a = buf + 2 * npx, *b = buf + 3 * npx, *cc = buf + 4 * npx;
  float *ba = buf + 5 * npx, *bb = buf + 6 * npx, *bc = buf + 7 * npx;
  float *dT = (float *)ctx->viewTaps.p, *hT = (float *)ctx->hViewTaps.p;
  int rc = MODSX_OK;
  if (detector_type == MODSX_DET_HESSIAN) {
    BlurBatch bt;
    memset(&bt, 0, sizeof bt);
    bt.j[0].src = img->d; bt.j[0].resp = res; bt.j[0].rows = rows; bt.j[0].cols = cols; bt.j[0].norm = norm;
    ctx->detCnt[mx::DT_HESSIAN] += launch_hessian(s, bt, 1, rows, cols);
  } else if (detector_type == MODSX_DET_DOG) {
    rc = blur_any(ctx, img->d, a, tmp, dT, hT, rows, cols, sigma);
    if (rc) return rc;
    launch_sub(s, img->d, a, res, npx);
  } else {
    launch_grad_products(s, img->d, rows, cols, a, b, cc);
    const int n = blur_ksize(sigma);
    // the three blurs share the taps: separate slices of the staging buffer so no upload waits for a previous one
    rc = blur_any(ctx, a, ba, tmp, dT, hT, rows, cols, sigma);
    if (!rc) rc = blur_any(ctx, b, bb, tmp, dT + 2 * n + 2, hT + 2 * n + 2, rows, cols, sigma);
    if (!rc) rc = blur_any(ctx, cc, bc, tmp, dT + 4 * n + 4, hT + 4 * n + 4, rows, cols, sigma);
    if (rc) return rc;
    launch_harris_combine(s, ba, bb, bc, (float)(0.6 * norm), res, npx);
  }
  MX_HIP(hipMemcpyAsync(out, res, npx * 4, hipMemcpyDeviceToHost, s));
  MX_HIP(hipStreamSynchronize(s));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

int modsx_resize_half(modsx_ctx *ctx, const modsx_image *img, float *out, int *orows, int *ocols) {
  NEED(ctx); NEED(img); NEED(orows); NEED(ocols);
  hipSetDevice(ctx->dev);
  const int dr = (int)lrint(img->rows * 0.5), dc = (int)lrint(img->cols * 0.5);
  *orows = dr; *ocols = dc;
  if (!out) return MODSX_OK;
  if (!ctx->scratchA.ensure((size_t)dr * dc * 4 + 4)) return MODSX_ERR_NOMEM;
  ResizeBatch rb;
  memset(&rb, 0, sizeof rb);
  rb.j[0].src = img->d; rb.j[0].dst = (float *)ctx->scratchA.p;
  rb.j[0].srows = img->rows; rb.j[0].scols = img->cols; rb.j[0].drows = dr; rb.j[0].dcols = dc;
  ctx->detCnt[mx::DT_RESIZE] += launch_resize_half(ctx->stream, rb, 1, dr, dc);
  MX_HIP(hipMemcpyAsync(out, ctx->scratchA.p, (size_t)dr * dc * 4, hipMemcpyDeviceToHost, ctx->stream));
  MX_HIP(hipStreamSynchronize(ctx->stream));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

int modsx_detect_affine_regions(const modsx_keypoint *kps, int n, int img_id, int det_type, modsx_region *out) {
  if (n < 0 || (n > 0 && (!kps || !out))) { mx::set_error("modsx_detect_affine_regions: bad argument"); return MODSX_ERR_ARG; }
  detect_affine_regions(kps, n, img_id, det_type, out);
  return n;
}

int modsx_detect_orientation(modsx_ctx *ctx, const modsx_image *img, const modsx_region *in, int n, double mrSize,
                             int patchSize, int doHalfSIFT, int maxAngNum, double th, int addUpRight,
                             modsx_region **out) {
  NEED(ctx); NEED(img); NEED(out);
  if (n < 0 || (n > 0 && !in)) { mx::set_error("modsx_detect_orientation: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_region> vin[1], vout[1];
  vin[0].assign(in, in + n);
  const modsx_image *imgs[1] = {img};
  int rc = detect_orientation_batch(ctx, imgs, 1, vin, mrSize, patchSize, doHalfSIFT, maxAngNum, th, addUpRight, vout);
  if (rc) return rc;
  *out = to_malloc(vout[0]);
  return (int)vout[0].size();
}

int modsx_reproject_regions(modsx_region *regs, int n, const double *H, int orig_w, int orig_h) {
  if (n < 0 || (n > 0 && !regs) || !H) { mx::set_error("modsx_reproject_regions: bad argument"); return MODSX_ERR_ARG; }
  return reproject_regions(regs, n, H, orig_w, orig_h);
}

int modsx_reproject_regions_touch_boundary(modsx_region *regs, int n, const double *H, int orig_w, int orig_h, double mrSize) {
  if (n < 0 || (n > 0 && !regs) || !H) { mx::set_error("modsx_reproject_regions_touch_boundary: bad argument"); return MODSX_ERR_ARG; }
  return reproject_regions_box(regs, n, H, orig_w, orig_h, mrSize);
}

int modsx_debug_reproject_certain_drop(const modsx_region *regs, int n, const double *H, int orig_w, int orig_h, double boxk,
                                       unsigned char *drop) {
  if (n < 0 || (n > 0 && (!regs || !drop)) || !H) { mx::set_error("modsx_debug_reproject_certain_drop: bad argument"); return MODSX_ERR_ARG; }
  reproject_certain_drop(regs, n, H, orig_w, orig_h, boxk, drop);
  return n;
}

int modsx_debug_orientation_counts(unsigned long long *launched, unsigned long long *skipped, int reset) {
  mx::orientation_counts(launched, skipped, reset != 0);
  return MODSX_OK;
}

int modsx_debug_orientation_launches(unsigned long long *lds_table, unsigned long long *global_table, int reset) {
  mx::orientation_launches(lds_table, global_table, reset != 0);
  return MODSX_OK;
}

int modsx_debug_views_counters(unsigned long long *views_fused, unsigned long long *groups, unsigned long long *rotated_pixels,
                               int reset) {
  mx::views_counters(views_fused, groups, rotated_pixels, reset != 0);
  return MODSX_OK;
}

int modsx_debug_view_plan(int rows, int cols, const modsx_view *view, int *geometry, double *rinv, double *winv) {
  if (rows < 1 || cols < 1 || !view || !geometry) { mx::set_error("modsx_debug_view_plan: bad argument"); return MODSX_ERR_ARG; }
  static const bool separate = getenv("MODSX_VIEWS_SEPARATE") && atoi(getenv("MODSX_VIEWS_SEPARATE"));
  mx::ViewPlan P;
  const int rc = mx::plan_view(rows, cols, *view, P);
  if (rc) return rc;
  const int g[8] = {P.identity, P.w_rot, P.h_rot, P.ow, P.oh, P.kx, P.ky, P.identity ? 0 : mx::view_fused_kind(P, separate)};
  for (int q = 0; q < 8; q++) geometry[q] = g[q];
  for (int q = 0; q < 6; q++) {
    if (rinv) rinv[q] = P.identity ? 0. : P.Rinv[q];
    if (winv) winv[q] = P.identity ? 0. : P.Winv[q];
  }
  return MODSX_OK;
}

int modsx_debug_views_groups(const int *source, const int *dims, const double *rinv, int n, int cap, int *group, int *order,
                             long long *totals) {
  if (n < 0 || (n > 0 && (!source || !dims || !rinv || !group || !order)) || !totals) {
    mx::set_error("modsx_debug_views_groups: bad argument"); return MODSX_ERR_ARG;
  }
  std::vector<mx::ViewPlan> plans(n);
  std::vector<mx::ViewGroupIn> in(n);
  for (int i = 0; i < n; i++) {
    plans[i].h_rot = dims[5 * i + 2]; plans[i].w_rot = dims[5 * i + 3];
    for (int q = 0; q < 6; q++) plans[i].Rinv[q] = rinv[6 * i + q];
    in[i] = {(const void *)(uintptr_t)(source[i] + 1), dims[5 * i], dims[5 * i + 1], &plans[i], dims[5 * i + 4]};
  }
  mx::ViewGrouping g;
  mx::group_views(in.data(), n, cap > 0 ? cap : mx::VIEW_GROUP_CAP, g);
  for (int i = 0; i < n; i++) { group[i] = g.group[i]; order[i] = g.order[i]; }
  totals[0] = g.nFused; totals[1] = g.nGroups; totals[2] = g.tiles; totals[3] = g.rotPx; totals[4] = g.rotPxAlone;
  return MODSX_OK;
}

int modsx_debug_synth_views(modsx_ctx *ctx, const modsx_image *const *imgs, const modsx_view *views, int n, modsx_image **out,
                            int *is_identity) {
  NEED(ctx);
  if (!imgs || !views || !out || !is_identity) { mx::set_error("modsx_debug_synth_views: null argument"); return MODSX_ERR_ARG; }
  if (n < 1 || n > mx::MAXB) { mx::set_error("batch size"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++) NEED(imgs[i]);
  hipSetDevice(ctx->dev);
  return synth_views_set(ctx, imgs, views, n, out, is_identity);
}

int modsx_orientation_tables(unsigned char *bin_table, unsigned short *index_raster, float *weight_raster,
                             unsigned short *index_lanes, float *weight_lanes, int *counts) {
  mx::OriTables t;
  const int rc = mx::orientation_tables_host(t);
  if (rc != MODSX_OK) return rc;
  if (bin_table) memcpy(bin_table, t.binTab.data(), 2049);
  if (index_raster) memcpy(index_raster, t.idxRaster.data(), mx::ORI_NV * sizeof(unsigned short));
  if (weight_raster) memcpy(weight_raster, t.wRaster.data(), mx::ORI_NV * sizeof(float));
  if (index_lanes) memcpy(index_lanes, t.idxLanes.data(), mx::ORI_NV * sizeof(unsigned short));
  if (weight_lanes) memcpy(weight_lanes, t.wLanes.data(), mx::ORI_NV * sizeof(float));
  if (counts) { counts[0] = t.nReal; counts[1] = mx::ORI_NV; counts[2] = mx::ORI_PSP; counts[3] = mx::ORI_LDS_TABLE_BELOW; }
  return MODSX_OK;
}

int modsx_debug_baumberg_geometry(int n, int W, int variant, int chunk, int *geometry) {
  NEED(geometry);
  const mx::BaumGeo g = mx::baumberg_geometry(n, W, variant, chunk);
  geometry[0] = g.kernel; geometry[1] = g.chunk; geometry[2] = g.nchunks; geometry[3] = g.grid;
  if (g.kernel < 0) { mx::set_error("modsx_debug_baumberg_geometry: no kernel for this window size / variant / chunk"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

int modsx_debug_baumberg_geometry_ctx(modsx_ctx *ctx, int n, int W, int variant, int chunk, int *geometry) {
  NEED(ctx); NEED(geometry);
  hipSetDevice(ctx->dev);
  return debug_baumberg_geometry(ctx, n, W, variant, chunk, geometry);
}

int modsx_debug_baumberg_variant(int W) { return mx::baumberg_production_variant(W); }

int modsx_debug_describe_lanes(int P, long *counts) {
  NEED(counts);
  if (P < 3) { mx::set_error("modsx_debug_describe_lanes: no such window"); return MODSX_ERR_ARG; }
  mx::DescSizePlan sp;
  const int rc = mx::describe_size_plan(P, sp);
  if (rc) return rc;
  mx::LaneCount k[4] = {};   // sampling taps, row filter, column filter of the fused small-window path, separate column filter
  const int NP = (sp.NC + 1) / 2;
  for (int r0 = 0; sp.rows0 > 0 && r0 < P; r0 += sp.rows0) {
    const int nr = std::min(sp.rows0, P - r0);
    mx::lanes_count_sampling(P, nr, mx::BF_T / 64, k[0]);
    mx::lanes_count_filter(nr * NP, k[1]);
  }
  if (sp.ro1 < 0) mx::lanes_count_filter(sp.NC * NP, k[2]);
  for (int ro0 = 0; sp.ro1 > 0 && ro0 < sp.NC; ro0 += sp.ro1) mx::lanes_count_filter(std::min(sp.ro1, sp.NC - ro0) * NP, k[3]);
  counts[0] = sp.ksize; counts[1] = sp.NC; counts[2] = sp.rows0; counts[3] = sp.ro1;
  for (int q = 0; q < 4; q++) { counts[4 + 3 * q] = k[q].useful; counts[5 + 3 * q] = k[q].issued; counts[6 + 3 * q] = k[q].issuedParent; }
  return MODSX_OK;
}

int modsx_debug_describe_lane_map(int rows, int nc, int *rule, int *map, int cap) {
  NEED(rule);
  if (rows < 1 || rows > 64) { mx::set_error("modsx_debug_describe_lane_map: a row pass has 1 .. 64 rows"); return MODSX_ERR_ARG; }
  constexpr mx::SrLaneTable T = mx::sr_lane_table();
  const int ncFull = mx::sr_table_cols(T.w[rows]), CP = mx::sr_stride(ncFull);
  rule[0] = ncFull; rule[1] = CP; rule[2] = mx::SR_PARK; rule[3] = 0; rule[4] = 0;
  if (nc == 0) return 0;
  if (nc < 0 || nc > ncFull || cap < 0 || (cap > 0 && !map)) { mx::set_error("modsx_debug_describe_lane_map: bad argument"); return MODSX_ERR_ARG; }
  const unsigned magic = mx::sr_table_magic(T.w[nc]);
  const int tot = rows * nc;
  rule[3] = (int)magic; rule[4] = mx::sr_slots(rows, nc);
  for (int e = 0; e < tot && e < cap; e++) {
    unsigned r, c;
    mx::sr_sample_rc((unsigned)e, nc, magic, r, c);
    map[3 * e] = (int)r; map[3 * e + 1] = (int)c; map[3 * e + 2] = (int)(r * (unsigned)CP + c);
  }
  return tot;
}

int modsx_debug_baumberg(modsx_ctx *ctx, const modsx_image *const *planes, int nplanes, const int *plane_of, const float *xyspd,
                         int n, const modsx_hessaff_params *par, int variant, int chunk, float *u, int *ok, int *iters,
                         int *geometry, int *handed_out) {
  NEED(ctx); NEED(par); NEED(geometry);
  if (n < 0 || nplanes < 0 || (nplanes > 0 && !planes) || (n > 0 && (!plane_of || !xyspd || !u || !ok || !iters))) {
    mx::set_error("modsx_debug_baumberg: bad argument"); return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  return debug_baumberg(ctx, planes, nplanes, plane_of, xyspd, n, *par, variant, chunk, u, ok, iters, geometry, handed_out);
}

int modsx_debug_check_borders(const float *tuples, int n, unsigned char *touch) {
  if (n < 0 || (n > 0 && (!tuples || !touch))) { mx::set_error("modsx_debug_check_borders: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++) {
    const float *t = tuples + 9 * (size_t)i;
    touch[i] = mx::check_borders((int)t[0], (int)t[1], t[2], t[3], t[4], t[5], t[6], t[7], (int)t[8], (int)t[8]) ? 1 : 0;
  }
  return n;
}

int modsx_describe_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  if (n < 0 || (n > 0 && !out)) { mx::set_error("modsx_describe_counters: bad argument"); return MODSX_ERR_ARG; }
  // the contexts that describe on this one's behalf count with it: the peer (the second image of a lone multi-view pair) and the
  // chains of half contexts of both (the further parts of a view list, engine_views.hip)
  long sum[mx::DC_ALL] = {0};
  for (modsx_ctx *head : {ctx, ctx->peer})
    for (modsx_ctx *c = head; c; c = c->half) {
      for (int q = 0; q < mx::DC_N; q++)
        if (q == mx::DC_MAX_CHUNKS) sum[q] = std::max(sum[q], c->descCnt[q]); else sum[q] += c->descCnt[q];
      // the device's word, read here and nowhere else: the description calls neither copy it nor wait for it
      unsigned now = 0;
      if (hipSetDevice(c->dev) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
          hipMemcpy(&now, c->dDescOrdered, 4, hipMemcpyDeviceToHost) != hipSuccess) {
        mx::set_error("modsx_describe_counters: reading the device counter failed"); return MODSX_ERR_DEVICE;
      }
      c->descOrderedTotal += (long)(unsigned)(now - c->descOrderedSeen);
      c->descOrderedSeen = now;
      sum[mx::DC_ORDERED_WG] += c->descOrderedTotal;
    }
  hipSetDevice(ctx->dev);
  for (int q = 0; q < n && q < mx::DC_ALL; q++) out[q] = sum[q];
  return mx::DC_ALL;
}

int modsx_describe_slim_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  if (n < 0 || (n > 0 && !out)) { mx::set_error("modsx_describe_slim_counters: bad argument"); return MODSX_ERR_ARG; }
  long sum[3] = {0, 0, 0};   // the same contexts as modsx_describe_counters
  for (modsx_ctx *head : {ctx, ctx->peer})
    for (modsx_ctx *c = head; c; c = c->half) {
      unsigned now = 0;
      if (hipSetDevice(c->dev) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
          hipMemcpy(&now, c->dDescOrdered + 1, 4, hipMemcpyDeviceToHost) != hipSuccess) {
        mx::set_error("modsx_describe_slim_counters: reading the device counter failed"); return MODSX_ERR_DEVICE;
      }
      c->descRedoTotal += (long)(unsigned)(now - c->descRedoSeen);
      c->descRedoSeen = now;
      sum[0] += c->descSlimCnt[0]; sum[1] += c->descSlimCnt[1]; sum[2] += c->descRedoTotal;
    }
  hipSetDevice(ctx->dev);
  for (int q = 0; q < n && q < 3; q++) out[q] = sum[q];
  return 3;
}

int modsx_blur_geometry(const int *rows, const int *cols, int n, int *geometry) {
  NEED(rows); NEED(cols); NEED(geometry);
  if (n < 1 || n > mx::MAXB) { mx::set_error("modsx_blur_geometry: 1 .. 32 planes"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++)
    if (rows[i] < 1 || cols[i] < 1 || !image_size_ok(rows[i], cols[i])) { mx::set_error("modsx_blur_geometry: plane size"); return MODSX_ERR_ARG; }
  const mx::BlurGeo g = mx::blur_geometry(rows, cols, n);
  geometry[0] = g.th; geometry[1] = g.tiles;
  return MODSX_OK;
}

int modsx_detect_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  if (n < 0 || (n > 0 && !out)) { mx::set_error("modsx_detect_counters: bad argument"); return MODSX_ERR_ARG; }
  long sum[mx::DT_N] = {0};
  for (const modsx_ctx *head : {(const modsx_ctx *)ctx, (const modsx_ctx *)ctx->peer})
    for (const modsx_ctx *c = head; c; c = c->half)
      for (int q = 0; q < mx::DT_N; q++)
        if (q != mx::DT_LAST_JOBS && q != mx::DT_LAST_TILES && q != mx::DT_LAST_ACCEPTED) sum[q] += c->detCnt[q];
  for (int q : {(int)mx::DT_LAST_JOBS, (int)mx::DT_LAST_TILES, (int)mx::DT_LAST_ACCEPTED}) sum[q] = ctx->detCnt[q];
  for (int q = 0; q < n && q < mx::DT_N; q++) out[q] = sum[q];
  return mx::DT_N;
}

int modsx_debug_pyramids(modsx_ctx *ctx, const modsx_image *const *imgs, int n, const modsx_hessaff_params *par, int *geometry,
                         float *planes, unsigned long long cap_floats, unsigned long long *need_floats) {
  NEED(ctx); NEED(imgs); NEED(par); NEED(geometry); NEED(need_floats);
  if (n < 1 || n > mx::MAXB) { mx::set_error("batch size"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++) NEED(imgs[i]);
  hipSetDevice(ctx->dev);
  return debug_pyramids(ctx, imgs, n, *par, geometry, planes, cap_floats, need_floats);
}

int modsx_debug_scan_levels(modsx_ctx *ctx, const float *resps, const float *blurs, int L, int rows, int cols,
                            const modsx_hessaff_params *par, modsx_candidate **cands, int *n_cands, modsx_sskp **out) {
  NEED(ctx); NEED(resps); NEED(blurs); NEED(par); NEED(cands); NEED(n_cands); NEED(out);
  static_assert(sizeof(modsx_candidate) == sizeof(mx::Candidate), "modsx_candidate is the device record");
  hipSetDevice(ctx->dev);
  std::vector<mx::Candidate> cd;
  std::vector<modsx_sskp> kp;
  int rc = debug_scan_levels(ctx, resps, blurs, L, rows, cols, *par, cd, kp);
  if (rc) return rc;
  modsx_candidate *m = (modsx_candidate *)malloc(std::max<size_t>(1, cd.size()) * sizeof(modsx_candidate));
  if (!m) return MODSX_ERR_NOMEM;
  if (!cd.empty()) memcpy(m, cd.data(), cd.size() * sizeof(modsx_candidate));
  *cands = m; *n_cands = (int)cd.size();
  *out = to_malloc(kp);
  return (int)kp.size();
}

int modsx_debug_detect_scalespace_batch(modsx_ctx *ctx, const modsx_image *const *imgs, int n, const modsx_hessaff_params *par,
                                        modsx_sskp **out, int *counts) {
  NEED(ctx); NEED(imgs); NEED(par); NEED(out); NEED(counts);
  if (n < 1 || n > mx::MAXB) { mx::set_error("batch size"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++) NEED(imgs[i]);
  hipSetDevice(ctx->dev);
  std::vector<modsx_sskp> k[mx::MAXB];
  int rc = detect_scalespace_batch(ctx, imgs, n, *par, k);
  if (rc) return rc;
  for (int i = 0; i < n; i++) { out[i] = to_malloc(k[i]); counts[i] = (int)k[i].size(); }
  return n;
}

int modsx_debug_describe_plan(const modsx_region *regs, const int *counts, int nimages, double mr_size, int fast_extraction,
                              unsigned long long arena_floats, long *counters, int n, long *cuts, int cap_cuts, int *n_cuts) {
  if (nimages < 0 || (nimages > 0 && !counts) || n < 0 || (n > 0 && !counters) || cap_cuts < 0 || (cap_cuts > 0 && !cuts) || !n_cuts) {
    mx::set_error("modsx_debug_describe_plan: bad argument"); return MODSX_ERR_ARG;
  }
  if (nimages > mx::MAXB) { mx::set_error("describe batch too large"); return MODSX_ERR_ARG; }
  std::vector<modsx_region> v[mx::MAXB];
  long first[mx::MAXB + 1] = {0};    // flat index of every image's first region
  for (int i = 0; i < nimages; i++) {
    if (counts[i] < 0 || (counts[i] > 0 && !regs)) { mx::set_error("modsx_debug_describe_plan: bad argument"); return MODSX_ERR_ARG; }
    v[i].assign(regs + first[i], regs + first[i] + counts[i]);
    first[i + 1] = first[i] + counts[i];
  }
  // describe_batch's loop (engine.hip) without its device half
  mx::HostMark hm;
  mx::DescBatch batch;
  batch.regs = v; batch.n = nimages; batch.mrSize = mr_size; batch.fast = fast_extraction;
  mx::DescCursor cur = mx::describe_windows(batch);
  long cnt[mx::DC_N] = {0};
  int chunkNo = 0, rc = MODSX_OK;
  *n_cuts = 0;
  cnt[mx::DC_CALLS]++;
  for (; cur.img < nimages; chunkNo++) {
    mx::DescChunkPlan cp;
    if (chunkNo) { if (*n_cuts < cap_cuts) cuts[*n_cuts] = first[cur.img] + (long)cur.reg; (*n_cuts)++; }
    rc = mx::describe_plan_chunk(batch, cur, (size_t)arena_floats, cp, hm);
    for (int q = 0; q < mx::DC_N; q++) cnt[q] += cp.cnt[q];
    if (rc) break;
    cur = cp.next;
  }
  if (!rc) cnt[mx::DC_MAX_CHUNKS] = chunkNo;
  for (int q = 0; q < n && q < mx::DC_N; q++) counters[q] = cnt[q];
  return rc;
}

int modsx_debug_describe_plan_slim(const modsx_region *regs, const int *counts, int nimages, double mr_size, int fast_extraction,
                                   unsigned long long arena_floats, unsigned char *slim, int cap, int *n_chunks) {
  if (nimages < 0 || (nimages > 0 && !counts) || cap < 0 || (cap > 0 && !slim) || !n_chunks) {
    mx::set_error("modsx_debug_describe_plan_slim: bad argument"); return MODSX_ERR_ARG;
  }
  if (nimages > mx::MAXB) { mx::set_error("describe batch too large"); return MODSX_ERR_ARG; }
  std::vector<modsx_region> v[mx::MAXB];
  size_t first = 0;
  for (int i = 0; i < nimages; i++) {
    if (counts[i] < 0 || (counts[i] > 0 && !regs)) { mx::set_error("modsx_debug_describe_plan_slim: bad argument"); return MODSX_ERR_ARG; }
    v[i].assign(regs + first, regs + first + counts[i]);
    first += (size_t)counts[i];
  }
  mx::HostMark hm;
  mx::DescBatch batch;
  batch.regs = v; batch.n = nimages; batch.mrSize = mr_size; batch.fast = fast_extraction;
  *n_chunks = 0;
  for (mx::DescCursor cur = mx::describe_windows(batch); cur.img < nimages; (*n_chunks)++) {
    mx::DescChunkPlan cp;
    const int rc = mx::describe_plan_chunk(batch, cur, (size_t)arena_floats, cp, hm);
    if (rc) return rc;
    if (*n_chunks < cap) slim[*n_chunks] = cp.slim ? 1 : 0;
    cur = cp.next;
  }
  return MODSX_OK;
}

int modsx_describe_regions(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                           int patchSize, int fast_extraction, int photoNorm, int desc_type, double maxBinValue,
                           float *desc) {
  NEED(ctx); NEED(img);
  if (n < 0 || (n > 0 && (!regs || !desc))) { mx::set_error("modsx_describe_regions: bad argument"); return MODSX_ERR_ARG; }
  if (desc_type < MODSX_DESC_SIFT || desc_type > MODSX_DESC_HALF_ROOT_SIFT) { mx::set_error("descriptor type"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_region> v[1];
  v[0].assign(regs, regs + n);
  const modsx_image *imgs[1] = {img};
  float *hosts[1] = {desc};
  int rc = describe_batch(ctx, imgs, 1, v, mrSize, patchSize, fast_extraction, photoNorm, desc_type, maxBinValue, hosts,
                          nullptr, nullptr);
  if (rc) return rc;
  return n;
}

int modsx_match_fginn(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, const double *pos2,
                      double ratio, double contradDist, int nn, modsx_tentative **out) {
  NEED(ctx); NEED(out);
  if (n1 < 0 || n2 < 0 || (n1 > 0 && !desc1) || (n2 > 0 && (!desc2 || !pos2))) { mx::set_error("modsx_match_fginn: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  int rc = match_host_desc(ctx, desc1, n1, desc2, n2, pos2, ratio, contradDist, nn, t);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}

int modsx_duplicate_filtering(const double *pts, const double *key, int T, double r, int do_sort, int *order,
                              unsigned char *keep) {
  if (T < 0 || (T > 0 && (!pts || !order || !keep))) { mx::set_error("modsx_duplicate_filtering: bad argument"); return MODSX_ERR_ARG; }
  return duplicate_filtering(pts, key, T, r, do_sort, order, keep);
}

int modsx_ransac_h(const double *u, int len, double th, double conf, int max_sam, double *H, unsigned char *inl,
                   int *data_out, int oriented_constraint, int doSymCheck, unsigned seed, double *score_J) {
  if (!u || !H || !inl || !data_out || len < 4) { mx::set_error("modsx_ransac_h: bad argument"); return MODSX_ERR_ARG; }
  return ransac_h(u, len, th, conf, max_sam, H, inl, data_out, oriented_constraint, doSymCheck, seed, score_J);
}

int modsx_ransac_h_errtype(const double *u, int len, double th, double conf, int max_sam, double *H, unsigned char *inl,
                           int *data_out, int oriented_constraint, int doSymCheck, int error_type, unsigned seed, double *score_J) {
  if (!u || !H || !inl || !data_out || len < 4 || error_type < 0 || error_type > 2) { mx::set_error("modsx_ransac_h_errtype: bad argument"); return MODSX_ERR_ARG; }
  return ransac_h(u, len, th, conf, max_sam, H, inl, data_out, oriented_constraint, doSymCheck, seed, score_J, error_type);
}

int modsx_ransac_f(const double *u, int len, double th, double conf, int max_sam, int do_lo, unsigned inl_limit,
                   int error_type, int doSymCheck, unsigned seed, double *F, unsigned char *inl, int *data_out) {
  if (!u || !F || !inl || !data_out || len < 8) { mx::set_error("modsx_ransac_f: bad argument"); return MODSX_ERR_ARG; }
  return ransac_f(u, len, th, conf, max_sam, F, inl, data_out, do_lo, inl_limit, error_type, doSymCheck, seed);
}

int modsx_loransac_f(const double *pts, const double *laf1, const double *laf2, int T, double err_threshold,
                     double confidence, int max_samples, int localOptimization, double LAFCoef, int doSymmCheck,
                     int error_type, unsigned seed, double *F, unsigned char *inl, unsigned char *keep, int *data_out) {
  if (!pts || !laf1 || !laf2 || !F || !inl || !keep || !data_out || T < 0) {
    mx::set_error("modsx_loransac_f: bad argument");
    return MODSX_ERR_ARG;
  }
  return loransac_f(pts, laf1, laf2, T, err_threshold, confidence, max_samples, localOptimization, LAFCoef, doSymmCheck,
                    error_type, seed, F, inl, keep, data_out);
}

int modsx_loransac_h(const double *pts, const double *laf1, const double *laf2, int T, double err_threshold,
                     double confidence, int max_samples, int localOptimization, double HLAFCoef, int doSymmCheck,
                     unsigned seed, double *H, double *Hraw, unsigned char *inl, unsigned char *keep, int *data_out) {
  if (T < 0 || !H || !Hraw || !data_out || (T > 0 && (!pts || !laf1 || !laf2 || !inl || !keep))) {
    mx::set_error("modsx_loransac_h: bad argument");
    return MODSX_ERR_ARG;
  }
  return loransac_h(pts, laf1, laf2, T, err_threshold, confidence, max_samples, localOptimization, HLAFCoef, doSymmCheck,
                    seed, H, Hraw, inl, keep, data_out);
}

int modsx_loransac_h_errtype(const double *pts, const double *laf1, const double *laf2, int T, double err_threshold,
                             double confidence, int max_samples, int localOptimization, double HLAFCoef, int doSymmCheck,
                             int error_type, unsigned seed, double *H, double *Hraw, unsigned char *inl, unsigned char *keep,
                             int *data_out) {
  if (T < 0 || !H || !Hraw || !data_out || (T > 0 && (!pts || !laf1 || !laf2 || !inl || !keep)) || error_type < 0 || error_type > 2) {
    mx::set_error("modsx_loransac_h_errtype: bad argument");
    return MODSX_ERR_ARG;
  }
  return loransac_h(pts, laf1, laf2, T, err_threshold, confidence, max_samples, localOptimization, HLAFCoef, doSymmCheck,
                    seed, H, Hraw, inl, keep, data_out, error_type);
}

// the consumer of the batch calls: DuplicateFiltering + LO-RANSAC of one matched pair, timed
static void verify_timed(mx::VerifyTask &t, const modsx_pair_params &pp) {
  hipSetDevice(t.dev);     // a new thread starts on device 0: the verifier's device-side loops belong on the producing context's GPU
  const auto v0 = std::chrono::steady_clock::now();
  mx::verify_tentatives(t.l1, t.l2, t.tents, pp, t.res);
  g_batch.add(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - v0).count());
}
// the caller's current HIP device is its own: worker 0 of the batch calls runs on the caller's thread and sets the contexts'.
// Every public batch entry holds exactly one.
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
  ~DeviceGuard() { if (dev >= 0) hipSetDevice(dev); }
};
// all contexts of a batch call search the same descriptor database, or none
static int same_fginn_db(modsx_ctx *const *ctxs, int n_ctx, const char *who) {
  for (int i = 1; i < n_ctx; i++)
    if (ctxs[i]->fginnDb != ctxs[0]->fginnDb) { mx::set_error(std::string(who) + ": all contexts of a call must have the same descriptor database attached, or none"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}
// the end of a batch call: n on success; a failed batch returns no results -- what the successful groups already own is released
static int batch_return(const mx::BatchError &err, modsx_pair_result *results, int n) {
  if (!err.rc) return n;
  for (int i = 0; i < n; i++) modsx_pair_result_release(&results[i]);
  mx::set_error(err.text);
  return err.rc;
}

int modsx_match_pair(modsx_ctx *ctx, const modsx_image *img1, const modsx_image *img2, const modsx_pair_params *par,
                     modsx_pair_result *res) {
  NEED(ctx); NEED(img1); NEED(img2); NEED(par); NEED(res);
  hipSetDevice(ctx->dev);
  return match_pair(ctx, img1, img2, *par, res);
}

int modsx_match_pairs(modsx_ctx *const *ctxs, int n_ctx, const modsx_image *const *imgs1,
                      const modsx_image *const *imgs2, int n_pairs, const modsx_pair_params *par,
                      modsx_pair_result *results) {
  NEED(ctxs); NEED(par); NEED(results);
  if (n_ctx <= 0 || n_pairs < 0 || (n_pairs > 0 && (!imgs1 || !imgs2))) { mx::set_error("modsx_match_pairs: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n_ctx; i++) NEED(ctxs[i]);
  { const int rc = same_fginn_db(ctxs, n_ctx, "modsx_match_pairs"); if (rc) return rc; }
  for (int i = 0; i < n_pairs; i++) memset(&results[i], 0, sizeof results[i]);   // no result owns arrays before its group ran
  const modsx_pair_params pp = *par;
  DeviceGuard restoreCallerDevice;
  // Every context takes up to PAIR_GROUP pairs at a time and runs their 2g images as one batch.  Verification (DuplicateFiltering +
  // LO-RANSAC, ~1.4 ms of host time per pair against ~0.9 ms of device time) runs on helper threads: the context's own thread goes
  // straight on to the next group, so its stream is idle only while the host prepares job tables, not while it runs RANSAC.
  const mx::BatchError err = mx::run_batch<mx::VerifyTask>(
      n_ctx, n_pairs, mx::PAIR_GROUP, verify_helper_cap(), g_batch,
      [&](int w, int i, int g, std::vector<mx::VerifyTask> &tasks) {
        hipSetDevice(ctxs[w]->dev);
        return match_pair_group(ctxs[w], imgs1 + i, imgs2 + i, g, pp, &results[i], &tasks);
      },
      [&](mx::VerifyTask &t) { verify_timed(t, pp); }, mx::last_error);
  return batch_return(err, results, n_pairs);
}

// modsx_match_pairs for multi-view pairs: every context takes one pair at a time (the pairs come off a shared counter), runs
// the view loop of both images and the match, and hands the tentatives to a helper thread for DuplicateFiltering +
// LO-RANSAC while its own thread goes on to the next pair -- a 31-view pair carries ~12 k tentatives and ~10 ms of host
// verification, during which the context's stream would otherwise sit idle.
int modsx_match_pairs_views(modsx_ctx *const *ctxs, int n_ctx, const modsx_image *const *imgs1, const modsx_image *const *imgs2,
                            int n_pairs, const modsx_view *views, int n_views, const modsx_pair_params *par,
                            modsx_pair_result *results) {
  NEED(ctxs); NEED(par); NEED(results); NEED(views);
  if (n_ctx <= 0 || n_views <= 0 || n_pairs < 0 || (n_pairs > 0 && (!imgs1 || !imgs2))) {
    mx::set_error("modsx_match_pairs_views: bad argument");
    return MODSX_ERR_ARG;
  }
  for (int i = 0; i < n_ctx; i++) NEED(ctxs[i]);
  { const int rc = same_fginn_db(ctxs, n_ctx, "modsx_match_pairs_views"); if (rc) return rc; }
  for (int i = 0; i < n_pairs; i++) memset(&results[i], 0, sizeof results[i]);
  const modsx_pair_params pp = *par;
  DeviceGuard restoreCallerDevice;
  const mx::BatchError err = mx::run_batch<mx::VerifyTask>(
      n_ctx, n_pairs, 1, verify_helper_cap(), g_batch,
      [&](int w, int i, int, std::vector<mx::VerifyTask> &tasks) {
        hipSetDevice(ctxs[w]->dev);
        tasks.emplace_back();
        return mx::match_pair_views(ctxs[w], imgs1[i], imgs2[i], views, n_views, pp, &results[i], &tasks.back());
      },
      [&](mx::VerifyTask &t) { verify_timed(t, pp); }, mx::last_error);
  return batch_return(err, results, n_pairs);
}

// ---- stored representations: one against many (engine_reps.hip) ---------------------------------------------------------------
// One round of MatchImgReps + verification of rep1 against n partners: the contexts take groups of up to MATCH_MAXB partners off
// a shared counter, a group costs one matcher launch set per class of sel; every partner's tentatives (tents[i], the classes of
// sel replaced, the others kept) are verified over the ordered class list `present`, on helper threads while the contexts go on.
// results[i] must own nothing or the arrays of an earlier round (released here).  The round is over when it returns.  The caller
// holds the DeviceGuard.
static mx::BatchError reps_round(modsx_ctx *const *ctxs, int n_ctx, const modsx_rep *rep1, const modsx_rep *const *reps2, int n,
                                 const modsx_rep_class_sel *sel, int nsel, const mx::RepClassList &present, const modsx_pair_params &pp,
                                 mx::RepTents *tents, modsx_pair_result *results) {
  return mx::run_batch<mx::VerifyTask>(
      n_ctx, n, mx::MATCH_MAXB, verify_helper_cap(), g_batch,
      [&](int w, int i, int g, std::vector<mx::VerifyTask> &tasks) {
        modsx_ctx *c = ctxs[w];
        hipSetDevice(c->dev);
        mx::RepTents *tp[mx::MATCH_MAXB];
        for (int k = 0; k < g; k++) tp[k] = &tents[i + k];
        const int rc = mx::reps_match_group(c, rep1, reps2 + i, g, sel, nsel, pp, tp);
        if (rc) return rc;
        tasks.resize(g);
        for (int k = 0; k < g; k++) {
          modsx_pair_result_release(&results[i + k]);
          mx::reps_verify_task(rep1, reps2[i + k], present, tents[i + k], &results[i + k], c->dev, tasks[k]);
        }
        return (int)MODSX_OK;
      },
      [&](mx::VerifyTask &t) { verify_timed(t, pp); }, mx::last_error);
}
static int reps_contexts_ok(modsx_ctx *const *ctxs, int n_ctx, const char *who) {
  if (!ctxs || n_ctx < 1) { mx::set_error(std::string(who) + ": at least one context is needed"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n_ctx; i++) if (!ctxs[i]) { mx::set_error(std::string(who) + ": null context"); return MODSX_ERR_ARG; }
  { const int rc = same_fginn_db(ctxs, n_ctx, who); if (rc) return rc; }
  for (int i = 1; i < n_ctx; i++)
    if (ctxs[i]->dev != ctxs[0]->dev) { mx::set_error(std::string(who) + ": the contexts must share one device (that of the representations)"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

int modsx_match_reps(modsx_ctx *const *ctxs, int n_ctx, const modsx_rep *rep1, const modsx_rep *const *reps2, int n,
                     const modsx_rep_class_sel *classes, int n_classes, const modsx_pair_params *par, modsx_pair_result *results) {
  { const int rc = reps_contexts_ok(ctxs, n_ctx, "modsx_match_reps"); if (rc) return rc; }
  NEED(rep1); NEED(par);
  if (n < 0 || n_classes < 0 || n_classes > mx::REP_CLASSES_MAX || (n > 0 && (!reps2 || !results)) || (n_classes > 0 && !classes)) {
    mx::set_error("modsx_match_reps: bad argument");
    return MODSX_ERR_ARG;
  }
  for (int i = 0; i < n; i++) NEED(reps2[i]);
  for (int i = 0; i <= n; i++)
    if ((i ? reps2[i - 1] : rep1)->dev != ctxs[0]->dev) { mx::set_error("modsx_match_reps: a representation lives on another device than the contexts"); return MODSX_ERR_ARG; }
  modsx_rep_class_sel sel[mx::REP_CLASSES_MAX];
  int nsel = 0;
  mx::RepClassList present;      // the classes that are verified, in the order GetCorresponcesVector concatenates them
  if (n_classes > 0) {
    for (int k = 0; k < n_classes; k++) {
      mx::RepClassId id;
      if (!mx::rep_class_id(classes[k].detector, classes[k].desc_type, &id)) {
        mx::set_error("modsx_match_reps: a class names a detector or descriptor type that does not exist"); return MODSX_ERR_ARG;
      }
      if (present.has(id)) { mx::set_error("modsx_match_reps: a class is listed twice"); return MODSX_ERR_ARG; }
      if (id.kind == mx::REP_BIN) {
        // a binary class: `ratio` is its DistanceThreshold; every partner is checked before any group is launched
        const int rc = mx::reps_bin_check("modsx_match_reps", ctxs[0], rep1, reps2, n, id.det, id.type, classes[k].ratio);
        if (rc) return rc;
      }
      present.add(id);
      sel[nsel++] = classes[k];
    }
  } else {
    mx::DescSet ds;
    { const int rd = mx::resolve_descs(*par, nullptr, ds); if (rd) return rd; }
    mx::rep_classes(present, 1u << mx::REP_U8 | 1u << mx::REP_F32);      // the binary classes are matched only when they are named
    for (int i = 0; i < present.n; i++) {
      const mx::RepClassId &id = present.k[i];
      if (mx::rep_class_regions(rep1, id).empty()) continue;   // no queries: no partner has tentatives in this class
      double ratio = par->match_ratio;
      for (int j = 0; j < ds.n && id.kind == mx::REP_U8; j++) if (ds.type[j] == id.type && ds.ratio[j] > 0) ratio = ds.ratio[j];
      sel[nsel].detector = mx::rep_class_detector(id); sel[nsel].desc_type = id.type; sel[nsel].ratio = ratio;
      nsel++;
    }
  }
  for (int i = 0; i < n; i++) memset(&results[i], 0, sizeof results[i]);
  if (n == 0) return 0;
  DeviceGuard restoreCallerDevice;
  std::vector<mx::RepTents> tents((size_t)n);
  return batch_return(reps_round(ctxs, n_ctx, rep1, reps2, n, sel, nsel, present, *par, tents.data(), results), results, n);
}

int modsx_match_one_to_many(modsx_ctx *const *ctxs, int n_ctx, const modsx_image *img1, const modsx_image *const *imgs2, int n,
                            const modsx_ladder_step *steps, int nsteps, int min_matches, const modsx_pair_params *par,
                            modsx_pair_result *results, int *steps_done) {
  { const int rc = reps_contexts_ok(ctxs, n_ctx, "modsx_match_one_to_many"); if (rc) return rc; }
  NEED(img1); NEED(steps); NEED(par);
  if (n < 0 || nsteps <= 0 || (n > 0 && (!imgs2 || !results))) { mx::set_error("modsx_match_one_to_many: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++) NEED(imgs2[i]);
  for (int s = 0; s < nsteps; s++)
    if (!steps[s].views || steps[s].nviews <= 0) { mx::set_error("modsx_match_one_to_many: empty step"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++) memset(&results[i], 0, sizeof results[i]);
  if (steps_done) *steps_done = 0;
  if (n == 0) return 0;
  DeviceGuard restoreCallerDevice;
  // image 0 of the call is img1, image i + 1 partner i: one representation each, freed before the call returns
  std::vector<modsx_rep *> reps((size_t)n + 1, nullptr);
  for (auto &r : reps) r = modsx_rep_create(ctxs[0]);
  std::vector<mx::RepTents> tents((size_t)n);
  mx::RepClassList u8Classes;      // the ladder carries the SIFT-family classes only
  mx::rep_classes(u8Classes, 1u << mx::REP_U8);
  mx::BatchError err;
  int step = 0;
  bool reached = false;
  for (; step < nsteps && !reached; step++) {
    // SynthDetectDescribeKeypoints + AddRegions of the step: the n + 1 images come off a shared counter
    err = mx::run_groups(
        n_ctx, n + 1, 1,
        [&](int w, int i, int) {
          hipSetDevice(ctxs[w]->dev);
          const int ra = mx::rep_add_views(ctxs[w], reps[i], i ? imgs2[i - 1] : img1, steps[step], *par);
          return ra < 0 ? ra : 0;
        },
        mx::last_error, [](int) {});
    if (err.rc) break;
    // MatchImgReps re-matches the classes of the step's detector with the step's ratios; the verified set comes from all classes
    mx::DescSet ds;
    err.rc = mx::resolve_descs(*par, &steps[step], ds);
    if (err.rc) { err.text = mx::last_error(); break; }
    modsx_rep_class_sel sel[MODSX_MAX_DESC];
    for (int j = 0; j < ds.n; j++) { sel[j].detector = steps[step].detector == MODSX_DET_MSER ? MODSX_DET_MSER : MODSX_DET_HESSIAN; sel[j].desc_type = ds.type[j]; sel[j].ratio = ds.ratio[j]; }
    err = reps_round(ctxs, n_ctx, reps[0], reps.data() + 1, n, sel, ds.n, u8Classes, *par, tents.data(), results);
    if (err.rc) break;
    for (int i = 0; i < n; i++) reached = reached || results[i].n_verified >= min_matches;
  }
  for (auto &r : reps) modsx_rep_free(ctxs[0], r);
  if (err.rc) return batch_return(err, results, n);
  if (steps_done) *steps_done = step;
  return n;
}

void modsx_pair_result_release(modsx_pair_result *res) {
  if (!res) return;
  free(res->tentatives); free(res->ransac_inlier); free(res->verified);
  res->tentatives = nullptr; res->ransac_inlier = nullptr; res->verified = nullptr;
}

int modsx_last_batch_verify(double *sum_ms, int *pairs, int *threads) {
  if (sum_ms) *sum_ms = g_batch.taskUs.load() / 1000.0;
  if (pairs) *pairs = g_batch.tasks.load();
  if (threads) *threads = g_batch.workers.load();
  return MODSX_OK;
}

int modsx_last_match_geometry(int *qs, int *fat, int *S, int *tiles_per_split, int *ntiles_ub) {
  mx::last_match_geometry(qs, fat, S, tiles_per_split, ntiles_ub);
  return MODSX_OK;
}

// verification time (DuplicateFiltering + LO-RANSAC + the LAF checks, wall of the verifying thread) of every pair of the last batch
// call, in completion order.  Written by the four batch entries as modsx_last_batch_verify is (modsx.h).
extern "C" __attribute__((visibility("default"))) int modsx_debug_last_batch_verify_each(double *ms, int cap) {
  std::lock_guard<std::mutex> lk(g_batch.eachMu);
  const int n = (int)g_batch.eachUs.size();
  for (int i = 0; i < n && i < cap; i++) ms[i] = g_batch.eachUs[i] / 1000.0;
  return n;
}

// CPU seconds (thread CPU clocks, not wall) the last batch call spent in the contexts' own threads (matching, and verifying once
// they are out of pairs) and in its verification helpers.  Written by the four batch entries as modsx_last_batch_verify is.
extern "C" __attribute__((visibility("default"))) int modsx_debug_last_batch_cpu(double *worker_s, double *helper_s) {
  if (worker_s) *worker_s = g_batch.cpuWorkerUs.load() / 1e6;
  if (helper_s) *helper_s = g_batch.cpuHelperUs.load() / 1e6;
  return MODSX_OK;
}

// 1: stage boundaries wait through the runtime (hipStreamSynchronize) right now, 0: through the context's flag word (engine.hip, MODSX_HOST_WAIT;
// `auto` follows the process' CPU load)
extern "C" __attribute__((visibility("default"))) int modsx_debug_host_wait_runtime() { return mx::host_wait_runtime() ? 1 : 0; }

int modsx_last_timings(modsx_ctx *ctx, double *ms6) {
  NEED(ctx); NEED(ms6);
  for (int i = 0; i < 6; i++) ms6[i] = ctx->timings[i];
  return MODSX_OK;
}

int modsx_set_vs_pars(const double *scale_set, int ns, const double *tilt_set, int nt, double phi_base,
                      double InitSigma, int doBlur, modsx_view *par, int cap, modsx_view *prev, int *nprev,
                      int cap_prev) {
  if (ns < 0 || nt < 0 || !par || !prev || !nprev || (ns > 0 && !scale_set) || (nt > 0 && !tilt_set)) {
    mx::set_error("modsx_set_vs_pars: bad argument");
    return MODSX_ERR_ARG;
  }
  return set_vs_pars(scale_set, ns, tilt_set, nt, phi_base, InitSigma, doBlur, par, cap, prev, nprev, cap_prev);
}

modsx_image *modsx_synth_view(modsx_ctx *ctx, const modsx_image *gray, const modsx_view *view, double *H9,
                              int *is_identity) {
  if (!ctx || !gray || !view || !H9 || !is_identity) { mx::set_error("modsx_synth_view: null argument"); return nullptr; }
  hipSetDevice(ctx->dev);
  modsx_image *out = nullptr;
  if (synth_view(ctx, gray, *view, &out, H9, is_identity) != MODSX_OK) return nullptr;
  return out;
}

int modsx_detect_describe_views(modsx_ctx *ctx, const modsx_image *img, const modsx_view *views, int nviews,
                                const modsx_pair_params *par, int view_begin, int view_step, modsx_region **regs,
                                float **desc, void *dev_desc_u8, long dev_cap, int *view_counts) {
  NEED(ctx); NEED(img); NEED(views); NEED(par); NEED(regs);
  if (nviews <= 0 || view_begin < 0) { mx::set_error("modsx_detect_describe_views: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_region> r;
  size_t cap = dev_desc_u8 ? (size_t)dev_cap : ((size_t)1 << 16);
  std::vector<int> counts(nviews, 0);
  int rc;
  for (;;) {
    if (!ctx->descAllF[0].ensure(cap * 512)) return MODSX_ERR_NOMEM;
    uint8_t *du8 = (uint8_t *)dev_desc_u8;
    if (!du8) { if (!ctx->descAllU8[0].ensure(cap * 128)) return MODSX_ERR_NOMEM; du8 = (uint8_t *)ctx->descAllU8[0].p; }
    rc = detect_describe_views(ctx, img, views, nviews, *par, view_begin, view_step, r, (float *)ctx->descAllF[0].p, du8,
                               cap, nullptr, counts.data());
    if (rc == MODSX_ERR_CAPACITY && !dev_desc_u8 && cap < ((size_t)1 << 24)) { cap *= 4; continue; }
    break;
  }
  if (rc) return rc;
  if (view_counts) memcpy(view_counts, counts.data(), sizeof(int) * nviews);
  if (view_step <= 1 && view_begin == 0) rebase_ids(r, counts.data(), nviews, 0);
  if (desc) {
    *desc = (float *)malloc(std::max<size_t>(1, r.size()) * 512);
    if (!r.empty()) {
      MX_HIP(hipMemcpyAsync(*desc, ctx->descAllF[0].p, r.size() * 512, hipMemcpyDeviceToHost, ctx->stream));
      MX_HIP(hipStreamSynchronize(ctx->stream));
    }
  }
  *regs = to_malloc(r);
  return (int)r.size();
}

int modsx_match_fginn_device(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2,
                             const double *pos2, double ratio, double contradDist, int nn, modsx_tentative **out) {
  NEED(ctx); NEED(out);
  if (n1 < 0 || n2 < 0 || (n1 > 0 && !dev_desc1_u8) || (n2 > 0 && (!dev_desc2_u8 || !pos2))) {
    mx::set_error("modsx_match_fginn_device: bad argument");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  int rc = match_device(ctx, (const uint8_t *)dev_desc1_u8, n1, (const uint8_t *)dev_desc2_u8, n2, pos2, ratio,
                        contradDist, nn, t);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}

// ---- the descriptor database of MatchFlannFGINNPlusDB --------------------------------------------------------------------------
modsx_db *modsx_db_create(modsx_ctx *ctx, const void *rows, long n, int dtype) {
  if (!ctx) { mx::set_error("modsx_db_create: null context"); return nullptr; }
  hipSetDevice(ctx->dev);
  mx::DbSet *s = db_create(ctx, rows, n, dtype);
  return reinterpret_cast<modsx_db *>(s);     // modsx_db holds exactly one DbSet
}
void modsx_db_free(modsx_ctx *ctx, modsx_db *db) {
  if (!db) return;
  if (ctx) {
    hipSetDevice(ctx->dev);
    if (ctx->fginnDb == &db->set) ctx->fginnDb = nullptr;     // freeing a database that is attached to the freeing context detaches it
  }
  db_free(&db->set);
}
long modsx_db_rows(const modsx_db *db) { return db ? db->set.rows : 0; }
int modsx_db_nearest(modsx_ctx *ctx, const modsx_db *db, const float *desc, int n, float *dmin) {
  NEED(ctx); NEED(db);
  if (n < 0 || (n > 0 && (!desc || !dmin))) { mx::set_error("modsx_db_nearest: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return db_nearest(ctx, db->set, desc, n, dmin);
}
static double *d2_to_malloc(const std::vector<double> &v) {
  double *p = (double *)malloc(sizeof(double) * std::max<size_t>(1, v.size()));
  if (!v.empty()) memcpy(p, v.data(), sizeof(double) * v.size());
  return p;
}
int modsx_match_fginn_db(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, const double *pos2,
                         double ratio, double contradDist, int nn, const modsx_db *db, modsx_tentative **out, double **d2byDB) {
  NEED(ctx); NEED(out);
  if (!db) { mx::set_error("modsx_match_fginn_db: null database"); return MODSX_ERR_ARG; }
  if (n1 < 0 || n2 < 0 || (n1 > 0 && !desc1) || (n2 > 0 && (!desc2 || !pos2))) { mx::set_error("modsx_match_fginn_db: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  std::vector<double> d2;
  int rc = match_host_desc(ctx, desc1, n1, desc2, n2, pos2, ratio, contradDist, nn, t, &db->set, &d2);
  if (rc) return rc;
  *out = to_malloc(t);
  if (d2byDB) *d2byDB = d2_to_malloc(d2);
  return (int)t.size();
}
int modsx_match_fginn_db_device(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2,
                                const double *pos2, double ratio, double contradDist, int nn, const modsx_db *db,
                                modsx_tentative **out, double **d2byDB) {
  NEED(ctx); NEED(out);
  if (!db) { mx::set_error("modsx_match_fginn_db_device: null database"); return MODSX_ERR_ARG; }
  if (n1 < 0 || n2 < 0 || (n1 > 0 && !dev_desc1_u8) || (n2 > 0 && (!dev_desc2_u8 || !pos2))) {
    mx::set_error("modsx_match_fginn_db_device: bad argument");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  std::vector<double> d2;
  int rc = match_device(ctx, (const uint8_t *)dev_desc1_u8, n1, (const uint8_t *)dev_desc2_u8, n2, pos2, ratio, contradDist, nn, t,
                        &db->set, &d2);
  if (rc) return rc;
  *out = to_malloc(t);
  if (d2byDB) *d2byDB = d2_to_malloc(d2);
  return (int)t.size();
}
int modsx_set_fginn_db(modsx_ctx *ctx, const modsx_db *db) {
  NEED(ctx);
  if (db && db->set.dev != ctx->dev) { mx::set_error("modsx_set_fginn_db: the descriptor database lives on another device"); return MODSX_ERR_ARG; }
  ctx->fginnDb = db ? &db->set : nullptr;
  return MODSX_OK;
}

// ---- MatchFLANNDistance: exact Hamming matching of binary descriptors (engine_hamming.hip) ---------------------------------------
int modsx_match_hamming(modsx_ctx *ctx, const void *desc1, int n1, const void *desc2, int n2, int nbytes, int dtype,
                        double distanceThreshold, modsx_tentative **out) {
  NEED(ctx); NEED(out);
  if ((n1 > 0 && !desc1) || (n2 > 0 && !desc2)) { mx::set_error("modsx_match_hamming: null descriptors"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  int rc = match_hamming_host(ctx, desc1, n1, desc2, n2, nbytes, dtype, distanceThreshold, t);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}
int modsx_match_hamming_device(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2, int nbytes,
                               double distanceThreshold, modsx_tentative **out) {
  NEED(ctx); NEED(out);
  if ((n1 > 0 && !dev_desc1_u8) || (n2 > 0 && !dev_desc2_u8)) { mx::set_error("modsx_match_hamming_device: null descriptors"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  int rc = match_hamming_device(ctx, (const uint8_t *)dev_desc1_u8, n1, (const uint8_t *)dev_desc2_u8, n2, nbytes, distanceThreshold, t);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}
int modsx_hamming_tentatives(const int *nn2, int n1, double distanceThreshold, modsx_tentative **out) {
  NEED(out);
  std::vector<modsx_tentative> t;
  int rc = hamming_tentatives(nn2, n1, distanceThreshold, t);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}
int modsx_debug_match_hamming(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2, int nbytes,
                              int splits, int *nn2, int *geometry) {
  NEED(ctx); NEED(dev_desc1_u8); NEED(dev_desc2_u8); NEED(nn2);
  int rc = hamming_check_args("modsx_debug_match_hamming", n1, n2, nbytes);
  if (rc) return rc;
  if (n1 < 1 || n2 < 2 || splits < 0) { mx::set_error("modsx_debug_match_hamming: needs n1 >= 1, n2 >= 2, splits >= 0"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return hamming_search_device(ctx, (const uint8_t *)dev_desc1_u8, n1, (const uint8_t *)dev_desc2_u8, n2, nbytes, splits, nn2, geometry);
}
int modsx_debug_hamming_geometry(int n1, int n2, int nbytes, int splits, int *geometry) {
  NEED(geometry);
  int rc = hamming_check_args("modsx_debug_hamming_geometry", n1, n2, nbytes);
  if (rc) return rc;
  if (n1 < 1 || n2 < 2 || splits < 0) { mx::set_error("modsx_debug_hamming_geometry: needs n1 >= 1, n2 >= 2, splits >= 0"); return MODSX_ERR_ARG; }
  const HammingGeo g = hamming_geometry(n1, n2, (nbytes + 3) / 4, splits);
  geometry[0] = g.tile; geometry[1] = g.S; geometry[2] = g.gx * g.S; geometry[3] = g.W;
  return MODSX_OK;
}
// under modsx_profile(ctx, 1): HIP-event times in ms of the last Hamming search of this context -- ms2[0] the two k_hamming_pack
// launches, ms2[1] k_hamming_2nn + k_hamming_merge (tools/bench_hamming.py)
extern "C" __attribute__((visibility("default"))) int modsx_debug_hamming_last_ms(modsx_ctx *ctx, double *ms2) {
  NEED(ctx); NEED(ms2);
  ms2[0] = ctx->hammingMs[0]; ms2[1] = ctx->hammingMs[1];
  return MODSX_OK;
}
int modsx_match_regions_hamming(modsx_ctx *ctx, const modsx_region *regs1, const void *desc1, int n1, const modsx_region *regs2,
                                const void *desc2, int n2, int nbytes, int dtype, double distanceThreshold, const modsx_pair_params *par,
                                modsx_pair_result *res) {
  NEED(ctx); NEED(par); NEED(res);
  if ((n1 > 0 && (!regs1 || !desc1)) || (n2 > 0 && (!regs2 || !desc2))) { mx::set_error("modsx_match_regions_hamming: null regions or descriptors"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return match_regions_hamming(ctx, regs1, desc1, n1, regs2, desc2, n2, nbytes, dtype, distanceThreshold, *par, res);
}

// ---- MatchFlannFGINN on f32 rows of any width (engine_fginn32.hip) ----------------------------------------------------------------
// the entries without `dist` are vector_dist = L2: the same calls with the default
static int fginn_f32_host(const char *fn, modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                          double ratio, double contradDist, int nn, int dist, modsx_tentative **out) {
  NEED(ctx); NEED(out);
  if ((n1 > 0 && !desc1) || (n2 > 0 && (!desc2 || !pos2))) { mx::set_error(std::string(fn) + ": null rows or positions"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  int rc = match_fginn32_host(ctx, desc1, n1, desc2, n2, dim, pos2, ratio, contradDist, nn, t, nullptr, dist);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}
static int fginn_f32_device(const char *fn, modsx_ctx *ctx, const void *dev_desc1, int n1, const void *dev_desc2, int n2, int dim,
                            const double *pos2, double ratio, double contradDist, int nn, int dist, modsx_tentative **out) {
  NEED(ctx); NEED(out);
  int rc = fginn32_check_args(fn, n1, n2, dim, ratio, nn);
  if (rc) return rc;
  if ((rc = fginn32_check_dist(fn, dist))) return rc;
  if ((n1 > 0 && !dev_desc1) || (n2 > 0 && (!dev_desc2 || !pos2))) { mx::set_error(std::string(fn) + ": null rows or positions"); return MODSX_ERR_ARG; }
  if (((uintptr_t)dev_desc1 | (uintptr_t)dev_desc2) & 3) { mx::set_error(std::string(fn) + ": rows must be 4-byte aligned"); return MODSX_ERR_ARG; }
  std::vector<modsx_tentative> t;
  if (n1 > 0 && n2 > 0) {
    hipSetDevice(ctx->dev);
    rc = match_fginn32_device(ctx, (const float *)dev_desc1, n1, (const float *)dev_desc2, n2, dim, pos2, ratio, contradDist, nn, t, nullptr, dist);
    if (rc) return rc;
  }
  *out = to_malloc(t);
  return (int)t.size();
}
int modsx_match_fginn_f32(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                          double ratio, double contradDist, int nn, modsx_tentative **out) {
  return fginn_f32_host("modsx_match_fginn_f32", ctx, desc1, n1, desc2, n2, dim, pos2, ratio, contradDist, nn, MODSX_DIST_L2, out);
}
int modsx_match_fginn_f32_dist(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                               double ratio, double contradDist, int nn, int dist, modsx_tentative **out) {
  return fginn_f32_host("modsx_match_fginn_f32_dist", ctx, desc1, n1, desc2, n2, dim, pos2, ratio, contradDist, nn, dist, out);
}
int modsx_match_fginn_f32_device(modsx_ctx *ctx, const void *dev_desc1, int n1, const void *dev_desc2, int n2, int dim, const double *pos2,
                                 double ratio, double contradDist, int nn, modsx_tentative **out) {
  return fginn_f32_device("modsx_match_fginn_f32_device", ctx, dev_desc1, n1, dev_desc2, n2, dim, pos2, ratio, contradDist, nn, MODSX_DIST_L2, out);
}
int modsx_match_fginn_f32_dist_device(modsx_ctx *ctx, const void *dev_desc1, int n1, const void *dev_desc2, int n2, int dim,
                                      const double *pos2, double ratio, double contradDist, int nn, int dist, modsx_tentative **out) {
  return fginn_f32_device("modsx_match_fginn_f32_dist_device", ctx, dev_desc1, n1, dev_desc2, n2, dim, pos2, ratio, contradDist, nn, dist, out);
}
static int fginn_regions(const char *fn, modsx_ctx *ctx, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2,
                         const float *desc2, int n2, int dim, const modsx_pair_params *par, int dist, bool bytes, modsx_pair_result *res) {
  NEED(ctx); NEED(par); NEED(res);
  if ((n1 > 0 && (!regs1 || !desc1)) || (n2 > 0 && (!regs2 || !desc2))) { mx::set_error(std::string(fn) + ": null regions or rows"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return match_regions_f32(ctx, regs1, desc1, n1, regs2, desc2, n2, dim, *par, res, dist, bytes);
}
int modsx_match_regions_f32(modsx_ctx *ctx, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2,
                            const float *desc2, int n2, int dim, const modsx_pair_params *par, modsx_pair_result *res) {
  return fginn_regions("modsx_match_regions_f32", ctx, regs1, desc1, n1, regs2, desc2, n2, dim, par, MODSX_DIST_L2, false, res);
}
int modsx_match_regions_f32_dist(modsx_ctx *ctx, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2,
                                 const float *desc2, int n2, int dim, const modsx_pair_params *par, int dist, modsx_pair_result *res) {
  return fginn_regions("modsx_match_regions_f32_dist", ctx, regs1, desc1, n1, regs2, desc2, n2, dim, par, dist, false, res);
}
int modsx_match_regions_l1(modsx_ctx *ctx, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2,
                           const float *desc2, int n2, const modsx_pair_params *par, modsx_pair_result *res) {
  return fginn_regions("modsx_match_regions_l1", ctx, regs1, desc1, n1, regs2, desc2, n2, 128, par, MODSX_DIST_L1, true, res);
}
// bytes: the L1 search on byte rows (modsx_debug_match_fginn_l1)
static int fginn_debug(const char *fn, modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                       double ratio, double contradDist, int nn, int dist, bool bytes, int splits, int stage_mask, unsigned long long *top4,
                       unsigned char *stage, int *geometry, int *counters, modsx_tentative **out) {
  NEED(ctx); NEED(desc1); NEED(desc2); NEED(pos2);
  if (n1 < 1 || n2 < 1 || splits < 0 || (stage_mask != 1 && stage_mask != 3)) {
    mx::set_error(std::string(fn) + ": needs n1 >= 1, n2 >= 1, splits >= 0 and a stage mask of 1 or 3");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  const Fginn32Tap tap = {splits, stage_mask, top4, stage, geometry, counters};
  std::vector<modsx_tentative> t;
  int rc = bytes ? match_fginn_l1_host(ctx, desc1, n1, desc2, n2, pos2, ratio, contradDist, nn, t, &tap)
                 : match_fginn32_host(ctx, desc1, n1, desc2, n2, dim, pos2, ratio, contradDist, nn, t, &tap, dist);
  if (rc) return rc;
  if (out) *out = to_malloc(t);
  return (int)t.size();
}
int modsx_debug_match_fginn_f32(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                                double ratio, double contradDist, int nn, int splits, int stage_mask, unsigned long long *top4,
                                unsigned char *stage, int *geometry, int *counters, modsx_tentative **out) {
  return fginn_debug("modsx_debug_match_fginn_f32", ctx, desc1, n1, desc2, n2, dim, pos2, ratio, contradDist, nn, MODSX_DIST_L2, false, splits, stage_mask,
                     top4, stage, geometry, counters, out);
}
int modsx_debug_match_fginn_f32_dist(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2,
                                     double ratio, double contradDist, int nn, int dist, int splits, int stage_mask, unsigned long long *top4,
                                     unsigned char *stage, int *geometry, int *counters, modsx_tentative **out) {
  return fginn_debug("modsx_debug_match_fginn_f32_dist", ctx, desc1, n1, desc2, n2, dim, pos2, ratio, contradDist, nn, dist, false, splits, stage_mask, top4,
                     stage, geometry, counters, out);
}
int modsx_debug_match_fginn_l1(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, const double *pos2, double ratio,
                               double contradDist, int nn, int splits, int stage_mask, unsigned long long *top4, unsigned char *stage,
                               int *geometry, int *counters, modsx_tentative **out) {
  return fginn_debug("modsx_debug_match_fginn_l1", ctx, desc1, n1, desc2, n2, 128, pos2, ratio, contradDist, nn, MODSX_DIST_L1, true, splits, stage_mask, top4,
                     stage, geometry, counters, out);
}
int modsx_match_fginn_l1(modsx_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, const double *pos2, double ratio,
                         double contradDist, int nn, modsx_tentative **out) {
  NEED(ctx); NEED(out);
  if ((n1 > 0 && !desc1) || (n2 > 0 && (!desc2 || !pos2))) { mx::set_error("modsx_match_fginn_l1: null rows or positions"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  int rc = match_fginn_l1_host(ctx, desc1, n1, desc2, n2, pos2, ratio, contradDist, nn, t);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}
int modsx_match_fginn_l1_device(modsx_ctx *ctx, const void *dev_desc1_u8, int n1, const void *dev_desc2_u8, int n2, const double *pos2,
                                double ratio, double contradDist, int nn, modsx_tentative **out) {
  NEED(ctx); NEED(out);
  int rc = fginn32_check_args("modsx_match_fginn_l1_device", n1, n2, 128, ratio, nn);
  if (rc) return rc;
  if ((n1 > 0 && !dev_desc1_u8) || (n2 > 0 && (!dev_desc2_u8 || !pos2))) { mx::set_error("modsx_match_fginn_l1_device: null rows or positions"); return MODSX_ERR_ARG; }
  std::vector<modsx_tentative> t;
  if (n1 > 0 && n2 > 0) {
    hipSetDevice(ctx->dev);
    rc = match_fginn_l1_device(ctx, (const uint8_t *)dev_desc1_u8, n1, (const uint8_t *)dev_desc2_u8, n2, pos2, ratio, contradDist, nn, t);
    if (rc) return rc;
  }
  *out = to_malloc(t);
  return (int)t.size();
}
int modsx_debug_fginn_l1_geometry(int n1, int n2, int splits, int *geometry) {
  NEED(geometry);
  int rc = fginn32_check_args("modsx_debug_fginn_l1_geometry", n1, n2, 128, 0.5, 2);
  if (rc) return rc;
  if (n1 < 1 || n2 < 1 || splits < 0) { mx::set_error("modsx_debug_fginn_l1_geometry: needs n1 >= 1, n2 >= 1, splits >= 0"); return MODSX_ERR_ARG; }
  return fginn_l1_geometry_report(n1, n2, splits, geometry);
}
int modsx_debug_fginn32_geometry(int n1, int n2, int dim, int splits, int *geometry) {
  NEED(geometry);
  int rc = fginn32_check_args("modsx_debug_fginn32_geometry", n1, n2, dim, 0.5, 2);
  if (rc) return rc;
  if (n1 < 1 || n2 < 1 || splits < 0) { mx::set_error("modsx_debug_fginn32_geometry: needs n1 >= 1, n2 >= 1, splits >= 0"); return MODSX_ERR_ARG; }
  return fginn32_geometry_report(n1, n2, dim, splits, geometry);
}
int modsx_debug_fginn32_dpass(const float *d0, const double *ratio, int n, float *dpass) {
  if (n < 0 || (n > 0 && (!d0 || !ratio || !dpass))) { mx::set_error("modsx_debug_fginn32_dpass: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++) {
    if (!(d0[i] >= 0.f) || isinf(d0[i]) || !(ratio[i] * ratio[i] >= 0)) { mx::set_error("modsx_debug_fginn32_dpass: d0 must be finite and >= 0, ratio not NaN"); return MODSX_ERR_ARG; }
    dpass[i] = fginn32_dpass(d0[i], ratio[i] * ratio[i]);
  }
  return MODSX_OK;
}
// under modsx_profile(ctx, 1): HIP-event times in ms of the last f32 FGINN search of this context -- ms2[0] the two k_f32_pack
// launches, ms2[1] k_f32_topk + k_f32_merge (tools/bench_fginn32.py) -- or of its last L1 search on byte rows: the two k_l1_pack
// launches, k_l1_topk + k_f32_merge (tools/bench_fginn_l1.py)
extern "C" __attribute__((visibility("default"))) int modsx_debug_fginn32_last_ms(modsx_ctx *ctx, double *ms2) {
  NEED(ctx); NEED(ms2);
  ms2[0] = ctx->fginn32Ms[0]; ms2[1] = ctx->fginn32Ms[1];
  return MODSX_OK;
}

int modsx_match_ladder(modsx_ctx *ctx, const modsx_image *img1, const modsx_image *img2,
                       const modsx_ladder_step *steps, int nsteps, int min_matches, const modsx_pair_params *par,
                       modsx_pair_result *res, int *steps_done) {
  NEED(ctx); NEED(img1); NEED(img2); NEED(steps); NEED(par); NEED(res);
  if (nsteps <= 0) { mx::set_error("modsx_match_ladder: nsteps"); return MODSX_ERR_ARG; }
  for (int s = 0; s < nsteps; s++)
    if (!steps[s].views || steps[s].nviews <= 0) { mx::set_error("modsx_match_ladder: empty step"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return match_ladder(ctx, img1, img2, steps, nsteps, min_matches, *par, res, steps_done);
}

int modsx_match_pair_views(modsx_ctx *ctx, const modsx_image *img1, const modsx_image *img2,
                           const modsx_view *views, int nviews, const modsx_pair_params *par,
                           modsx_pair_result *res) {
  NEED(ctx); NEED(img1); NEED(img2); NEED(views); NEED(par); NEED(res);
  if (nviews <= 0) { mx::set_error("modsx_match_pair_views: nviews"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return match_pair_views(ctx, img1, img2, views, nviews, *par, res);
}

void modsx_default_mser_params(modsx_mser_params *p) {
  // build/config_iter_mods_cviu.ini:4-12; extremaParams.h:66-82
  memset(p, 0, sizeof *p);
  p->min_size = 30; p->max_area = 0.05; p->min_margin = 8; p->relative = 0;
  p->mode = MODSX_FIXED_TH; p->reg_number = 500; p->rel_threshold = -1; p->rel_reg_number = -1;
}

int modsx_detect_msers(modsx_ctx *ctx, const modsx_image *img, const modsx_mser_params *par, double tilt, double zoom,
                       modsx_keypoint **out) {
  NEED(ctx); NEED(img); NEED(par); NEED(out);
  if (par->min_size < 1 || !(par->max_area > 0)) { mx::set_error("modsx_detect_msers: parameters"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  const size_t n = (size_t)img->rows * img->cols;
  if (!ctx->misc.ensure(n + 16)) return MODSX_ERR_NOMEM;
  launch_trunc_u8(ctx->stream, img->d, (uint8_t *)ctx->misc.p, n);
  std::vector<uint8_t> host(n);
  MX_HIP(hipMemcpyAsync(host.data(), ctx->misc.p, n, hipMemcpyDeviceToHost, ctx->stream));
  MX_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<modsx_keypoint> k;
  int rc = detect_msers_host(host.data(), img->rows, img->cols, *par, tilt, zoom, k);
  if (rc) return rc;
  *out = (modsx_keypoint *)malloc(sizeof(modsx_keypoint) * std::max<size_t>(1, k.size()));
  if (!*out) { mx::set_error("out of memory"); return MODSX_ERR_NOMEM; }
  if (!k.empty()) memcpy(*out, k.data(), sizeof(modsx_keypoint) * k.size());
  return (int)k.size();
}

int modsx_detect_msers_u8(const unsigned char *gray, int rows, int cols, const modsx_mser_params *par, double tilt,
                          double zoom, modsx_keypoint **out) {
  if (!gray || !par || !out || rows <= 0 || cols <= 0 || par->min_size < 1 || !(par->max_area > 0)) {
    mx::set_error("modsx_detect_msers_u8: bad argument");
    return MODSX_ERR_ARG;
  }
  std::vector<modsx_keypoint> k;
  int rc = detect_msers_host(gray, rows, cols, *par, tilt, zoom, k);
  if (rc) return rc;
  *out = (modsx_keypoint *)malloc(sizeof(modsx_keypoint) * std::max<size_t>(1, k.size()));
  if (!*out) { mx::set_error("out of memory"); return MODSX_ERR_NOMEM; }
  if (!k.empty()) memcpy(*out, k.data(), sizeof(modsx_keypoint) * k.size());
  return (int)k.size();
}

// The host half of the MSER view loop without a device (test aid): DetectMSERs of n u8 views as the engine runs them -- 2 n (view,
// polarity) tasks on the host pool that share a view's bin sort.  counts[i] = keys of view i; *out = the views' keys one after the
// other (modsx_free).  Returns the total or a negative status.
extern "C" __attribute__((visibility("default"))) int modsx_debug_msers_views_u8(const unsigned char *const *gray, const int *rows, const int *cols,
                                                                                  int n, const modsx_mser_params *par, const double *tilts,
                                                                                  const double *zooms, int *counts, modsx_keypoint **out) {
  if (!gray || !rows || !cols || n <= 0 || n > mx::MAXB || !par || !tilts || !zooms || !counts || !out) { mx::set_error("modsx_debug_msers_views_u8: bad argument"); return MODSX_ERR_ARG; }
  std::vector<modsx_keypoint> k[mx::MAXB];
  int rc = mx::detect_msers_views(gray, rows, cols, n, *par, tilts, zooms, k);
  if (rc) return rc;
  size_t total = 0;
  for (int i = 0; i < n; i++) { counts[i] = (int)k[i].size(); total += k[i].size(); }
  *out = (modsx_keypoint *)malloc(sizeof(modsx_keypoint) * std::max<size_t>(1, total));
  if (!*out) { mx::set_error("out of memory"); return MODSX_ERR_NOMEM; }
  size_t at = 0;
  for (int i = 0; i < n; i++) { if (!k[i].empty()) memcpy(*out + at, k[i].data(), sizeof(modsx_keypoint) * k[i].size()); at += k[i].size(); }
  return (int)total;
}

// The device half of the MSER view loop on its own (test aid): the n f32 views go to the context's view scratch as they are --
// no modsx_image_upload, which refuses images of one row or one column -- and through mser_front, the function the view loop
// calls, with the device sort on.
int modsx_debug_mser_front(modsx_ctx *ctx, const float *const *views_host, const int *rows, const int *cols, int n,
                           unsigned char *u8, int *start, int *order) {
  NEED(ctx); NEED(views_host); NEED(rows); NEED(cols); NEED(u8); NEED(start); NEED(order);
  if (n < 1 || n > mx::MAXB) { mx::set_error("modsx_debug_mser_front: 1 .. 32 views"); return MODSX_ERR_ARG; }
  size_t npxAll = 0;
  for (int i = 0; i < n; i++) {
    // the sorted offsets (r + 1) * (cols + 2) + c + 1 and the level starts are ints
    if (!views_host[i] || rows[i] < 1 || cols[i] < 1 || ((size_t)rows[i] + 2) * ((size_t)cols[i] + 2) > 0x7fffffffu) {
      mx::set_error("modsx_debug_mser_front: bad view"); return MODSX_ERR_ARG;
    }
    npxAll += (size_t)rows[i] * cols[i];
  }
  if (npxAll > 0x7fffffffu) { mx::set_error("modsx_debug_mser_front: too many pixels"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  CtxBusy busy(ctx);
  const float *dv[mx::MAXB];
  for (int i = 0; i < n; i++) {
    const size_t b = (size_t)rows[i] * cols[i] * 4;
    if (!ctx->viewImg[i].ensure(b)) return MODSX_ERR_NOMEM;
    MX_HIP(hipMemcpyAsync(ctx->viewImg[i].p, views_host[i], b, hipMemcpyHostToDevice, ctx->stream));
    dv[i] = (const float *)ctx->viewImg[i].p;
  }
  mx::MserFront mf;
  const int rc = mx::mser_front(ctx, dv, rows, cols, n, true, mf);
  if (rc) return rc;
  size_t at = 0;
  for (int i = 0; i < n; i++) {
    const size_t npx = (size_t)rows[i] * cols[i];
    memcpy(u8 + at, mf.u8[i], npx);
    memcpy(order + at, mf.order[i], npx * 4);
    memcpy(start + (size_t)i * 257, mf.start[i], 257 * 4);
    at += npx;
  }
  return MODSX_OK;
}

int modsx_save_regions(const char *path, const modsx_region_class *classes, int nclasses) {
  if (!path || !classes || nclasses <= 0) { mx::set_error("modsx_save_regions: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < nclasses; i++) {
    const modsx_region_class &c = classes[i];
    if (!c.det_name || !c.desc_name || c.n < 0 || c.dim < 0 || c.stride < c.dim || (c.n > 0 && (!c.regs || (c.dim > 0 && !c.desc)))) {
      mx::set_error("modsx_save_regions: bad class");
      return MODSX_ERR_ARG;
    }
  }
  return save_regions(path, classes, nclasses);
}

int modsx_load_regions(const char *path, const char *det_name, const char *desc_name, modsx_region **regs, float **desc,
                       int *dim, char *found_det, char *found_desc) {
  if (!path || !regs || !desc || !dim) { mx::set_error("modsx_load_regions: bad argument"); return MODSX_ERR_ARG; }
  std::vector<modsx_region> r;
  std::vector<float> d;
  std::string fd, fs;
  int rc;
  try { rc = load_regions(path, det_name, desc_name, r, d, dim, &fd, &fs); }
  catch (const std::exception &e) { mx::set_error(std::string("modsx_load_regions: ") + e.what()); return MODSX_ERR_NOMEM; }
  if (rc) return rc;
  *regs = (modsx_region *)malloc(sizeof(modsx_region) * std::max<size_t>(1, r.size()));
  *desc = (float *)malloc(sizeof(float) * std::max<size_t>(1, d.size()));
  if (!*regs || !*desc) { free(*regs); free(*desc); mx::set_error("out of memory"); return MODSX_ERR_NOMEM; }
  if (!r.empty()) memcpy(*regs, r.data(), sizeof(modsx_region) * r.size());
  if (!d.empty()) memcpy(*desc, d.data(), sizeof(float) * d.size());
  if (found_det) { strncpy(found_det, fd.c_str(), 63); found_det[63] = 0; }
  if (found_desc) { strncpy(found_desc, fs.c_str(), 63); found_desc[63] = 0; }
  return (int)r.size();
}

int modsx_profile(modsx_ctx *ctx, int enable) {
  NEED(ctx);
  prof_reset(ctx, enable != 0);
  return MODSX_OK;
}

// ---- the descriptors of normalised patches: their common argument check, call and counter read-out ----
#define PATCH_ARGS(fn, bad)                                                                                      \
  do {                                                                                                           \
    if (n < 0 || (bad)) { mx::set_error(fn ": bad argument"); return MODSX_ERR_ARG; }                            \
    if (patchSize != 41) { mx::set_error(fn ": patchSize must be 41"); return MODSX_ERR_ARG; }                   \
  } while (0)
// the engine call on the context's device; n rows on success
#define RETURN_ROWS(call)          \
  do {                             \
    hipSetDevice(ctx->dev);        \
    const int rc = (call);         \
    return rc ? rc : n;            \
  } while (0)
static int read_counters(const char *fn, const long *counters, int len, long *out, int n) {
  if (n < 0 || (n > 0 && !out)) { mx::set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
  for (int q = 0; q < n && q < len; q++) out[q] = counters[q];
  return len;
}

// ---- normalised patches and LIOP (engine_liop.hip) ----
int modsx_extract_patches(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize,
                          int fast_extraction, int photoNorm, float *patches) {
  NEED(ctx); NEED(img);
  PATCH_ARGS("modsx_extract_patches", !regs || !patches);
  RETURN_ROWS(extract_patches(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, patches, false));
}
int modsx_extract_patches_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                 int patchSize, int fast_extraction, int photoNorm, void *dev_patches) {
  NEED(ctx); NEED(img);
  PATCH_ARGS("modsx_extract_patches_device", !regs || !dev_patches || ((uintptr_t)dev_patches & 3));
  RETURN_ROWS(extract_patches(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, (float *)dev_patches, true));
}
int modsx_liop_patches(modsx_ctx *ctx, const float *patches, int n, int patchSize, float *desc) {
  NEED(ctx);
  PATCH_ARGS("modsx_liop_patches", !patches || !desc);
  RETURN_ROWS(liop_patches(ctx, patches, n, patchSize, desc, false, nullptr, nullptr));
}
int modsx_liop_patches_device(modsx_ctx *ctx, const void *dev_patches, int n, int patchSize, void *dev_desc) {
  NEED(ctx);
  PATCH_ARGS("modsx_liop_patches_device", !dev_patches || !dev_desc || (((uintptr_t)dev_patches | (uintptr_t)dev_desc) & 3));
  RETURN_ROWS(liop_patches(ctx, (const float *)dev_patches, n, patchSize, (float *)dev_desc, true, nullptr, nullptr));
}
int modsx_describe_regions_liop(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                int patchSize, int fast_extraction, int photoNorm, float *desc) {
  NEED(ctx); NEED(img);
  PATCH_ARGS("modsx_describe_regions_liop", !regs || !desc);
  RETURN_ROWS(describe_regions_liop(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, desc, false));
}
int modsx_describe_regions_liop_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                       int patchSize, int fast_extraction, int photoNorm, void *dev_desc) {
  NEED(ctx); NEED(img);
  PATCH_ARGS("modsx_describe_regions_liop_device", !regs || !dev_desc || ((uintptr_t)dev_desc & 3));
  RETURN_ROWS(describe_regions_liop(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, (float *)dev_desc, true));
}
int modsx_liop_tables(int patchSize, int *pixels, double *sx, double *sy, int cap) {
  if (cap < 0) { mx::set_error("modsx_liop_tables: bad argument"); return MODSX_ERR_ARG; }
  return liop_tables(patchSize, pixels, sx, sy, cap);
}
int modsx_debug_liop(modsx_ctx *ctx, const float *patches, int n, int patchSize, float *desc, int *path, int *perm) {
  NEED(ctx);
  PATCH_ARGS("modsx_debug_liop", !patches || !desc || !path || !perm);
  RETURN_ROWS(liop_patches(ctx, patches, n, patchSize, desc, false, path, perm));
}
int modsx_liop_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_liop_counters", ctx->liopCounters, 4, out, n);
}

// ---- raw SIFT histograms, the f32 SIFT norm and DSP-SIFT (engine_dsp.hip) ----
int modsx_describe_regions_raw(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize,
                               int fast_extraction, int photoNorm, float *hist) {
  NEED(ctx); NEED(img);
  PATCH_ARGS("modsx_describe_regions_raw", !regs || !hist);
  RETURN_ROWS(describe_regions_raw(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, hist, false));
}
int modsx_describe_regions_raw_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                      int patchSize, int fast_extraction, int photoNorm, void *dev_hist) {
  NEED(ctx); NEED(img);
  PATCH_ARGS("modsx_describe_regions_raw_device", !regs || !dev_hist || ((uintptr_t)dev_hist & 3));
  RETURN_ROWS(describe_regions_raw(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, (float *)dev_hist, true));
}
int modsx_sift_norm_rows(modsx_ctx *ctx, const float *rows, int n, double maxBinValue, float *out) {
  NEED(ctx);
  if (n < 0 || !rows || !out) { mx::set_error("modsx_sift_norm_rows: bad argument"); return MODSX_ERR_ARG; }
  RETURN_ROWS(sift_norm_rows(ctx, rows, n, maxBinValue, out, false));
}
int modsx_sift_norm_rows_device(modsx_ctx *ctx, const void *dev_rows, int n, double maxBinValue, void *dev_out) {
  NEED(ctx);
  if (n < 0 || !dev_rows || !dev_out || (((uintptr_t)dev_rows | (uintptr_t)dev_out) & 3)) {
    mx::set_error("modsx_sift_norm_rows_device: bad argument");
    return MODSX_ERR_ARG;
  }
  RETURN_ROWS(sift_norm_rows(ctx, (const float *)dev_rows, n, maxBinValue, (float *)dev_out, true));
}
int modsx_describe_regions_dspsift(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                   int patchSize, int fast_extraction, int photoNorm, int numScales, double startCoef, double endCoef,
                                   double maxBinValue, float *desc) {
  NEED(ctx); NEED(img);
  PATCH_ARGS("modsx_describe_regions_dspsift", !regs || !desc);
  RETURN_ROWS(describe_regions_dspsift(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, numScales, startCoef,
                                          endCoef, maxBinValue, desc, false));
}
int modsx_describe_regions_dspsift_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                          int patchSize, int fast_extraction, int photoNorm, int numScales, double startCoef,
                                          double endCoef, double maxBinValue, void *dev_desc) {
  NEED(ctx); NEED(img);
  PATCH_ARGS("modsx_describe_regions_dspsift_device", !regs || !dev_desc || ((uintptr_t)dev_desc & 3));
  RETURN_ROWS(describe_regions_dspsift(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, numScales, startCoef,
                                          endCoef, maxBinValue, (float *)dev_desc, true));
}
int modsx_dsp_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_dsp_counters", ctx->dspCounters, 3, out, n);
}

// ---- SURF (engine_surf.hip) ----
#define SURF_ARGS(fn, bad)                                                \
  do {                                                                    \
    PATCH_ARGS(fn, bad);                                                   \
    if (surf_check_args(fn, patchSize, mrSize)) return MODSX_ERR_ARG;        \
  } while (0)
int modsx_surf_patches(modsx_ctx *ctx, const float *patches, int n, int patchSize, double mrSize, float *desc) {
  NEED(ctx);
  SURF_ARGS("modsx_surf_patches", !patches || !desc);
  RETURN_ROWS(surf_patches(ctx, patches, n, mrSize, desc, false));
}
int modsx_surf_patches_device(modsx_ctx *ctx, const void *dev_patches, int n, int patchSize, double mrSize, void *dev_desc) {
  NEED(ctx);
  SURF_ARGS("modsx_surf_patches_device", !dev_patches || !dev_desc || (((uintptr_t)dev_patches | (uintptr_t)dev_desc) & 3));
  RETURN_ROWS(surf_patches(ctx, (const float *)dev_patches, n, mrSize, (float *)dev_desc, true));
}
int modsx_describe_regions_surf(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                int patchSize, int fast_extraction, int photoNorm, float *desc) {
  NEED(ctx); NEED(img);
  SURF_ARGS("modsx_describe_regions_surf", !regs || !desc);
  RETURN_ROWS(describe_regions_surf(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, desc, false));
}
int modsx_describe_regions_surf_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                       int patchSize, int fast_extraction, int photoNorm, void *dev_desc) {
  NEED(ctx); NEED(img);
  SURF_ARGS("modsx_describe_regions_surf_device", !regs || !dev_desc || ((uintptr_t)dev_desc & 3));
  RETURN_ROWS(describe_regions_surf(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, (float *)dev_desc, true));
}
int modsx_surf_tables(int patchSize, double mrSize, int *sample_x24, int *sample_y24, float *w1, float *w2, int *haar_size) {
  return surf_tables(patchSize, mrSize, sample_x24, sample_y24, w1, w2, haar_size);
}
int modsx_surf_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_surf_counters", ctx->surfCounters, 3, out, n);
}

// ---- the SURF detector (engine_surfdet.hip) ----
int modsx_surfdet_normalise(const modsx_surfdet_params *par, modsx_surfdet_params *out) {
  NEED(par); NEED(out);
  *out = surfdet_normalise(*par);
  return MODSX_OK;
}
int modsx_surfdet_geometry(int rows, int cols, const modsx_surfdet_params *par, int *layers) {
  NEED(par);
  return surfdet_geometry("modsx_surfdet_geometry", rows, cols, *par, layers);
}
int modsx_surf_regions(const modsx_keypoint *kps, int n, int img_id, modsx_region *out) {
  if (n < 0 || (n > 0 && (!kps || !out))) { mx::set_error("modsx_surf_regions: bad argument"); return MODSX_ERR_ARG; }
  surf_regions(kps, n, img_id, out);
  return n;
}
int modsx_detect_surf_batch(modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_surfdet_params *par,
                            modsx_keypoint **out, int *counts) {
  NEED(ctx); NEED(par); NEED(out);
  if (n_imgs < 0 || (n_imgs > 0 && (!imgs || !counts))) { mx::set_error("modsx_detect_surf_batch: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n_imgs; i++) NEED(imgs[i]);
  hipSetDevice(ctx->dev);
  std::vector<std::vector<modsx_keypoint>> k(n_imgs);
  const int rc = detect_surf_batch(ctx, imgs, n_imgs, *par, k.data());
  if (rc) return rc;
  std::vector<modsx_keypoint> all;
  for (int i = 0; i < n_imgs; i++) { counts[i] = (int)k[i].size(); all.insert(all.end(), k[i].begin(), k[i].end()); }
  *out = to_malloc(all);
  return (int)all.size();
}
int modsx_detect_surf(modsx_ctx *ctx, const modsx_image *img, const modsx_surfdet_params *par, modsx_keypoint **out) {
  NEED(ctx); NEED(img); NEED(par); NEED(out);
  int count = 0;
  const modsx_image *imgs[1] = {img};
  return modsx_detect_surf_batch(ctx, imgs, 1, par, out, &count);
}
int modsx_debug_surfdet(modsx_ctx *ctx, const modsx_image *img, const modsx_surfdet_params *par, float *integral, int *layers, float *resp,
                        unsigned char *lap, int *ext, double *dD, double *H, double *x, int *accepted, int *laplacian, int cap_ext,
                        int *n_ext) {
  NEED(ctx); NEED(img); NEED(par); NEED(integral); NEED(layers); NEED(resp); NEED(lap); NEED(n_ext);
  if (cap_ext < 0 || (cap_ext > 0 && (!ext || !dD || !H || !x || !accepted || !laplacian))) {
    mx::set_error("modsx_debug_surfdet: bad argument");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  return debug_surfdet(ctx, img, *par, integral, layers, resp, lap, ext, dD, H, x, accepted, laplacian, cap_ext, n_ext);
}
int modsx_surfdet_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_surfdet_counters", ctx->sdCounters, 5, out, n);
}

// ---- the KAZE detector (engine_kaze.hip) ----
void modsx_default_kaze_params(modsx_kaze_params *p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->omax = 4; p->nsublevels = 4; p->soffset = 1.6f; p->derivative_factor = 1.5f; p->dthreshold = 0.001f; p->min_dthreshold = 0.00001f;
  p->kcontrast_percentile = 0.7f; p->kcontrast_nbins = 300; p->descriptor = 5; p->diffusivity = 1;
}
int modsx_kaze_geometry(int rows, int cols, const modsx_kaze_params *par, int *levels, float *sigmas, float *tau, int *tiles, int *omax) {
  NEED(par);
  std::vector<KazeLevel> lv;
  const int n = kaze_geometry("modsx_kaze_geometry", rows, cols, *par, lv, omax);
  if (n < 0) return n;
  for (int i = 0; i < n; i++) {
    const KazeLevel &L = lv[i];
    if (levels) {
      const int row[8] = {L.octave, L.sublevel, L.rows, L.cols, L.sigma_size, L.ksize, L.dsize, L.nsteps};
      memcpy(levels + 8 * i, row, sizeof row);
    }
    if (sigmas) { sigmas[2 * i] = L.esigma; sigmas[2 * i + 1] = L.etime; }
    if (tau)
      for (int k = 0; k < MODSX_KAZE_MAX_TAU; k++) tau[(size_t)i * MODSX_KAZE_MAX_TAU + k] = k < L.nsteps ? L.tau[k] : 0.f;
  }
  if (tiles) { tiles[0] = KZ_TW; tiles[1] = KZ_TH; tiles[2] = KZ_TILE; tiles[3] = KZ_MAX_S; }
  return n;
}
int modsx_kaze_regions(const modsx_keypoint *kps, int n, int img_id, modsx_region *out) {
  if (n < 0 || (n > 0 && (!kps || !out))) { mx::set_error("modsx_kaze_regions: bad argument"); return MODSX_ERR_ARG; }
  kaze_regions(kps, n, img_id, out);
  return n;
}
int modsx_detect_kaze_batch(modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_kaze_params *par,
                            modsx_keypoint **out, int *counts) {
  NEED(ctx); NEED(par); NEED(out);
  if (n_imgs < 0 || (n_imgs > 0 && (!imgs || !counts))) { mx::set_error("modsx_detect_kaze_batch: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n_imgs; i++) NEED(imgs[i]);
  hipSetDevice(ctx->dev);
  std::vector<std::vector<modsx_keypoint>> k(n_imgs);
  const int rc = detect_kaze_batch(ctx, imgs, n_imgs, *par, k.data());
  if (rc) return rc;
  std::vector<modsx_keypoint> all;
  for (int i = 0; i < n_imgs; i++) { counts[i] = (int)k[i].size(); all.insert(all.end(), k[i].begin(), k[i].end()); }
  *out = to_malloc(all);
  return (int)all.size();
}
int modsx_detect_kaze(modsx_ctx *ctx, const modsx_image *img, const modsx_kaze_params *par, modsx_keypoint **out) {
  NEED(ctx); NEED(img); NEED(par); NEED(out);
  int count = 0;
  const modsx_image *imgs[1] = {img};
  return modsx_detect_kaze_batch(ctx, imgs, 1, par, out, &count);
}
static void kaze_lists_out(const KazeLists &L, int *raw, float *rawv, modsx_kaze_point *aux, modsx_kaze_point *upper, modsx_kaze_point *fin,
                           int cap, int *counts) {
  counts[0] = (int)L.rawv.size(); counts[1] = (int)L.aux.size(); counts[2] = (int)L.upper.size(); counts[3] = (int)L.final.size();
  const size_t c = (size_t)cap;
  if (cap > 0) {
    memcpy(raw, L.raw.data(), std::min(c, L.rawv.size()) * 3 * sizeof(int));
    memcpy(rawv, L.rawv.data(), std::min(c, L.rawv.size()) * sizeof(float));
    memcpy(aux, L.aux.data(), std::min(c, L.aux.size()) * sizeof(modsx_kaze_point));
    memcpy(upper, L.upper.data(), std::min(c, L.upper.size()) * sizeof(modsx_kaze_point));
    memcpy(fin, L.final.data(), std::min(c, L.final.size()) * sizeof(modsx_kaze_point));
  }
}
int modsx_debug_kaze(modsx_ctx *ctx, const modsx_image *img, const modsx_kaze_params *par, float *kc, long *hist, float *Lt, float *Lsmooth,
                     float *Lflow, float *Ldet, int *raw, float *rawv, modsx_kaze_point *aux, modsx_kaze_point *upper,
                     modsx_kaze_point *fin, int cap, int *counts) {
  NEED(ctx); NEED(img); NEED(par); NEED(kc); NEED(hist); NEED(Lt); NEED(Lsmooth); NEED(Lflow); NEED(Ldet); NEED(counts);
  if (cap < 0 || (cap > 0 && (!raw || !rawv || !aux || !upper || !fin))) { mx::set_error("modsx_debug_kaze: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  KazeLists L;
  const KazeTap tap = {kc, hist, Lt, Lsmooth, Lflow, Ldet, &L};
  const int rc = debug_kaze(ctx, img, *par, tap);
  if (rc < 0) return rc;
  kaze_lists_out(L, raw, rawv, aux, upper, fin, cap, counts);
  return rc;
}
int modsx_debug_kaze_scan(modsx_ctx *ctx, int rows, int cols, const modsx_kaze_params *par, const float *ldet, int *raw, float *rawv,
                          modsx_kaze_point *aux, modsx_kaze_point *upper, modsx_kaze_point *fin, int cap, int *counts) {
  NEED(ctx); NEED(par); NEED(ldet); NEED(counts);
  if (cap < 0 || (cap > 0 && (!raw || !rawv || !aux || !upper || !fin))) { mx::set_error("modsx_debug_kaze_scan: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  KazeLists L;
  const int rc = debug_kaze_scan(ctx, rows, cols, *par, ldet, L);
  if (rc < 0) return rc;
  kaze_lists_out(L, raw, rawv, aux, upper, fin, cap, counts);
  return rc;
}
int modsx_kaze_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_kaze_counters", ctx->kzCounters, 9, out, n);
}

// ---- external affine adaptation, DetectAffineShape (engine_detect.hip) ----
void modsx_default_affshape_params(modsx_affshape_params *p) {
  if (!p) return;
  // AffineShapeParams(), detectors/affinedetectors/affine.h:52-63
  p->maxIterations = 16;            // :54
  p->smmWindowSize = 19;            // :58
  p->convergenceThreshold = 0.05f;  // :56
  p->affBmbrgMethod = 0;            // :61 AFF_BMBRG_SMM
}
int modsx_affshape_jobs(const modsx_region *in, int n, int cols, int rows, float *ratio, int *res, unsigned char *border) {
  return affshape_jobs("modsx_affshape_jobs", in, n, cols, rows, ratio, res, border);
}
// what the three entries check before they look at the context: the parameters, the counts and every region's values (against
// the images where they are given); total = the regions in all
static int affshape_args(const char *fn, const modsx_image *const *imgs, int n_imgs, const modsx_region *in, const int *counts,
                         const modsx_affshape_params *par, long *total) {
  if (!par) { mx::set_error(std::string(fn) + ": null argument: par"); return MODSX_ERR_ARG; }
  int rc = affshape_check(fn, *par);
  if (rc) return rc;
  if (n_imgs < 0 || (n_imgs > 0 && !counts)) { mx::set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
  *total = 0;
  for (int i = 0; i < n_imgs; i++) {
    if (counts[i] < 0 || (counts[i] > 0 && !in)) { mx::set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
    const modsx_image *im = imgs ? imgs[i] : nullptr;
    rc = affshape_jobs(fn, in + *total, counts[i], im ? im->cols : 4, im ? im->rows : 4, nullptr, nullptr, nullptr);
    if (rc < 0) return rc;
    *total += counts[i];
  }
  return MODSX_OK;
}
int modsx_detect_affine_shape_batch(modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_region *in, const int *counts,
                                    const modsx_affshape_params *par, modsx_region **out, int *out_counts) {
  const char *fn = "modsx_detect_affine_shape_batch";
  NEED(out);
  long total = 0;
  int rc = affshape_args(fn, imgs, n_imgs, in, counts, par, &total);
  if (rc) return rc;
  if (n_imgs > 0 && !out_counts) { mx::set_error(std::string(fn) + ": null argument: out_counts"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n_imgs; i++) out_counts[i] = 0;
  std::vector<modsx_region> all;
  if (total == 0 || par->maxIterations <= 0) { *out = to_malloc(all); return 0; }
  NEED(ctx); NEED(imgs);
  for (int i = 0; i < n_imgs; i++) NEED(imgs[i]);
  hipSetDevice(ctx->dev);
  std::vector<std::vector<modsx_region>> r(n_imgs);
  rc = affine_shape_batch(ctx, fn, imgs, n_imgs, in, counts, *par, -1, r.data(), nullptr);
  if (rc < 0) return rc;
  for (int i = 0; i < n_imgs; i++) { out_counts[i] = (int)r[i].size(); all.insert(all.end(), r[i].begin(), r[i].end()); }
  *out = to_malloc(all);
  return (int)all.size();
}
int modsx_detect_affine_shape(modsx_ctx *ctx, const modsx_image *img, const modsx_region *in, int n, const modsx_affshape_params *par,
                              modsx_region **out) {
  int count = 0;
  const modsx_image *imgs[1] = {img};
  if (n < 0) { mx::set_error("modsx_detect_affine_shape: bad argument"); return MODSX_ERR_ARG; }
  return modsx_detect_affine_shape_batch(ctx, imgs, 1, in, &n, par, out, &count);
}
int modsx_debug_affine_shape(modsx_ctx *ctx, const modsx_image *const *imgs, int n_imgs, const modsx_region *in, const int *counts,
                             const modsx_affshape_params *par, int variant, unsigned char *border, float *u, int *ok, int *iters,
                             int *geometry) {
  const char *fn = "modsx_debug_affine_shape";
  NEED(ctx); NEED(geometry);
  long total = 0;
  int rc = affshape_args(fn, imgs, n_imgs, in, counts, par, &total);
  if (rc) return rc;
  if (n_imgs > 0) NEED(imgs);
  for (int i = 0; i < n_imgs; i++) NEED(imgs[i]);
  if (total > 0 && (!border || !u || !ok || !iters)) { mx::set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
  if (variant < -1 || variant > 3) { mx::set_error(std::string(fn) + ": variant must be -1 .. 3"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  const AffShapeReport rep = {border, u, ok, iters, geometry};
  return affine_shape_batch(ctx, fn, imgs, n_imgs, in, counts, *par, variant, nullptr, &rep);
}
int modsx_affshape_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_affshape_counters", ctx->affshapeCounters, 6, out, n);
}

// ---- CLAHE (engine_clahe.hip) ----
void modsx_default_clahe_params(modsx_clahe_params *p) {
  if (!p) return;
  // what every driver sets: createCLAHE(); setClipLimit(4), mods.cpp:139-189 (createCLAHE's own defaults: clip 40, 8 x 8 tiles)
  p->clip_limit = 4.0;
  p->tiles_x = 8; p->tiles_y = 8;
  p->variant = 0;
}
int modsx_clahe_geometry(int rows, int cols, const modsx_clahe_params *par, int *out) {
  NEED(par); NEED(out);
  ClaheGeo g;
  const int rc = clahe_geometry("modsx_clahe_geometry", rows, cols, *par, g);
  if (rc) return rc;
  int bits;
  memcpy(&bits, &g.lutScale, 4);
  const int v[9] = {g.tileW, g.tileH, g.padW, g.padH, g.clipLimit, bits, g.strips, g.stripRows, g.applyBlocks};
  memcpy(out, v, sizeof v);
  return 9;
}
int modsx_image_clahe_batch(modsx_ctx *ctx, const modsx_image *const *in, modsx_image *const *out, int n, const modsx_clahe_params *par) {
  const char *fn = "modsx_image_clahe_batch";
  NEED(par);
  int rc = clahe_check(fn, *par);
  if (rc) return rc;
  if (n < 0) { mx::set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
  if (n == 0) return MODSX_OK;
  NEED(ctx); NEED(in); NEED(out);
  for (int i = 0; i < n; i++) { NEED(in[i]); NEED(out[i]); }
  hipSetDevice(ctx->dev);
  return clahe_batch(ctx, fn, in, out, n, *par, nullptr, nullptr);
}
int modsx_image_clahe(modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par, modsx_image *out) {
  const char *fn = "modsx_image_clahe";
  NEED(par);
  int rc = clahe_check(fn, *par);
  if (rc) return rc;
  NEED(ctx); NEED(in); NEED(out);
  hipSetDevice(ctx->dev);
  return clahe_batch(ctx, fn, &in, &out, 1, *par, nullptr, nullptr);
}
modsx_image *modsx_image_clahe_new(modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par) {
  const char *fn = "modsx_image_clahe_new";
  if (!par || clahe_check(fn, *par)) { if (!par) mx::set_error(std::string(fn) + ": null argument: par"); return nullptr; }
  if (!ctx || !in) { mx::set_error(std::string(fn) + ": null argument"); return nullptr; }
  hipSetDevice(ctx->dev);
  modsx_image *im = new modsx_image();
  im->rows = in->rows; im->cols = in->cols; im->owned = true; im->d = nullptr;
  if (hipMalloc(&im->d, (size_t)in->rows * in->cols * 4) != hipSuccess) { mx::set_error("hipMalloc image"); delete im; return nullptr; }
  if (clahe_batch(ctx, fn, &in, &im, 1, *par, nullptr, nullptr) != MODSX_OK) { hipFree(im->d); delete im; return nullptr; }
  return im;
}
int modsx_debug_clahe(modsx_ctx *ctx, const modsx_image *in, const modsx_clahe_params *par, int *hist, unsigned char *lut) {
  const char *fn = "modsx_debug_clahe";
  NEED(par);
  int rc = clahe_check(fn, *par);
  if (rc) return rc;
  NEED(ctx); NEED(in);
  hipSetDevice(ctx->dev);
  return clahe_batch(ctx, fn, &in, nullptr, 1, *par, hist, lut);
}
// under modsx_profile(ctx, 1): HIP-event times in ms of the three launches of this context's last CLAHE call or batch --
// k_clahe_hist, k_clahe_lut, k_clahe_apply (tools/bench_clahe.py)
extern "C" __attribute__((visibility("default"))) int modsx_debug_clahe_last_ms(modsx_ctx *ctx, double *ms3) {
  NEED(ctx); NEED(ms3);
  for (int i = 0; i < 3; i++) ms3[i] = ctx->claheMs[i];
  return MODSX_OK;
}
int modsx_clahe_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_clahe_counters", ctx->claheCounters, 6, out, n);
}

// ---- the learned-descriptor front end (engine_caffe.hip) ----
void modsx_default_caffe_params(modsx_caffe_params *p) {
  if (!p) return;
  p->mrSize = 3.0 * sqrt(3.0);      // PatchExtractionParams
  p->patchSize = 41;
  p->mean[0] = 104; p->mean[1] = 117; p->mean[2] = 123;      // MeanB, MeanG, MeanR
}
// what both patch entries check before they look at the context
static int caffe_args(const char *fn, const modsx_image *const *planes, int n_planes, const modsx_region *regs, int n,
                      const modsx_caffe_params *par, const void *blob) {
  if (!par) { mx::set_error(std::string(fn) + ": null argument: par"); return MODSX_ERR_ARG; }
  const int rc = caffe_check(fn, *par);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!regs || !blob))) { mx::set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
  if (n_planes != 1 && n_planes != 3) { mx::set_error(std::string(fn) + ": 1 (gray) or 3 (B, G, R) planes"); return MODSX_ERR_ARG; }
  if (!planes) { mx::set_error(std::string(fn) + ": null argument: planes"); return MODSX_ERR_ARG; }
  for (int q = 0; q < n_planes; q++)
    if (!planes[q]) { mx::set_error(std::string(fn) + ": null argument: a plane"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}
int modsx_caffe_patches(modsx_ctx *ctx, const modsx_image *const *planes, int n_planes, const modsx_region *regs, int n,
                        const modsx_caffe_params *par, float *blob, unsigned char *flags) {
  const char *fn = "modsx_caffe_patches";
  const int rc = caffe_args(fn, planes, n_planes, regs, n, par, blob);
  if (rc) return rc;
  NEED(ctx);
  RETURN_ROWS(caffe_patches(ctx, fn, planes, n_planes, regs, n, *par, blob, false, flags));
}
int modsx_caffe_patches_device(modsx_ctx *ctx, const modsx_image *const *planes, int n_planes, const modsx_region *regs, int n,
                               const modsx_caffe_params *par, void *dev_blob, unsigned char *flags) {
  const char *fn = "modsx_caffe_patches_device";
  const int rc = caffe_args(fn, planes, n_planes, regs, n, par, dev_blob);
  if (rc) return rc;
  if ((uintptr_t)dev_blob & 3) { mx::set_error(std::string(fn) + ": the blob is not 4-byte aligned"); return MODSX_ERR_ARG; }
  NEED(ctx);
  RETURN_ROWS(caffe_patches(ctx, fn, planes, n_planes, regs, n, *par, (float *)dev_blob, true, flags));
}
int modsx_caffe_jobs(const modsx_region *regs, int n, const modsx_caffe_params *par, int rows, int cols, float *out) {
  const char *fn = "modsx_caffe_jobs";
  NEED(par);
  const int rc = caffe_check(fn, *par);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!regs || !out)) || rows < 2 || cols < 2) { mx::set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
  std::vector<CaffeJob> jobs(n);
  caffe_jobs(regs, n, *par, rows, cols, jobs.data());
  for (int i = 0; i < n; i++) {
    const CaffeJob &j = jobs[i];
    const float v[8] = {j.sc, j.x, j.y, j.a11, j.a12, j.a21, j.a22, j.touch ? 1.f : 0.f};
    memcpy(out + 8 * (size_t)i, v, sizeof v);
  }
  return n;
}
int modsx_debug_caffe_geometry(int n, int patchSize, int *out) {
  NEED(out);
  modsx_caffe_params p;
  modsx_default_caffe_params(&p);
  p.patchSize = patchSize;
  const int rc = caffe_check("modsx_debug_caffe_geometry", p);
  if (rc) return rc;
  if (n < 0) { mx::set_error("modsx_debug_caffe_geometry: bad argument"); return MODSX_ERR_ARG; }
  const CaffeGeo g = caffe_geometry(patchSize);
  const int v[7] = {8 * ((n + 7) / 8), g.waves, g.chunks, g.chunkCols, g.stride, g.planeBytes, 3 * g.planeBytes};
  memcpy(out, v, sizeof v);
  return 7;
}
int modsx_caffe_norm_rows(modsx_ctx *ctx, const float *rows, int n, int dim, int norm, float *out) {
  const char *fn = "modsx_caffe_norm_rows";
  const int rc = caffe_norm_check(fn, n, dim, norm);
  if (rc) return rc;
  if (n > 0 && (!rows || !out)) { mx::set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
  NEED(ctx);
  RETURN_ROWS(caffe_norm_rows(ctx, fn, rows, n, dim, norm, out, false));
}
int modsx_caffe_norm_rows_device(modsx_ctx *ctx, const void *dev_rows, int n, int dim, int norm, void *dev_out) {
  const char *fn = "modsx_caffe_norm_rows_device";
  const int rc = caffe_norm_check(fn, n, dim, norm);
  if (rc) return rc;
  if ((n > 0 && (!dev_rows || !dev_out)) || (((uintptr_t)dev_rows | (uintptr_t)dev_out) & 3)) {
    mx::set_error(std::string(fn) + ": bad argument");
    return MODSX_ERR_ARG;
  }
  NEED(ctx);
  RETURN_ROWS(caffe_norm_rows(ctx, fn, (const float *)dev_rows, n, dim, norm, (float *)dev_out, true));
}
int modsx_caffe_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_caffe_counters", ctx->caffeCounters, 4, out, n);
}

// ---- DAISY (engine_daisy.hip) ----
#define DAISY_ARGS(fn, bad)                                                                         \
  do {                                                                                                \
    PATCH_ARGS(fn, bad);                                                                               \
    if (daisy_check_args(fn, patchSize, rad, radq, thq, histq, nrm_type)) return MODSX_ERR_ARG;      \
  } while (0)
int modsx_daisy_dim(int radq, int thq, int histq) { return daisy_dim(radq, thq, histq); }
int modsx_daisy_patches(modsx_ctx *ctx, const float *patches, int n, int patchSize, int rad, int radq, int thq, int histq, int nrm_type,
                        float *desc) {
  NEED(ctx);
  DAISY_ARGS("modsx_daisy_patches", !patches || !desc);
  RETURN_ROWS(daisy_patches(ctx, patches, n, rad, radq, thq, nrm_type, desc, false));
}
int modsx_daisy_patches_device(modsx_ctx *ctx, const void *dev_patches, int n, int patchSize, int rad, int radq, int thq, int histq,
                               int nrm_type, void *dev_desc) {
  NEED(ctx);
  DAISY_ARGS("modsx_daisy_patches_device", !dev_patches || !dev_desc || (((uintptr_t)dev_patches | (uintptr_t)dev_desc) & 3));
  RETURN_ROWS(daisy_patches(ctx, (const float *)dev_patches, n, rad, radq, thq, nrm_type, (float *)dev_desc, true));
}
int modsx_describe_regions_daisy(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize,
                                 int fast_extraction, int photoNorm, int rad, int radq, int thq, int histq, int nrm_type, float *desc) {
  NEED(ctx); NEED(img);
  DAISY_ARGS("modsx_describe_regions_daisy", !regs || !desc);
  RETURN_ROWS(describe_regions_daisy(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, rad, radq, thq, nrm_type, desc,
                                        false));
}
int modsx_describe_regions_daisy_device(modsx_ctx *ctx, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                                        int patchSize, int fast_extraction, int photoNorm, int rad, int radq, int thq, int histq,
                                        int nrm_type, void *dev_desc) {
  NEED(ctx); NEED(img);
  DAISY_ARGS("modsx_describe_regions_daisy_device", !regs || !dev_desc || ((uintptr_t)dev_desc & 3));
  RETURN_ROWS(describe_regions_daisy(ctx, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, rad, radq, thq, nrm_type,
                                        (float *)dev_desc, true));
}
int modsx_daisy_tables(int rad, int radq, int thq, int histq, float *k5, float *kos8, float *zin8, int *fsz, float *taps, int *selected,
                       int *state, int *base, float *w) {
  return daisy_tables(rad, radq, thq, histq, k5, kos8, zin8, fsz, taps, selected, state, base, w);
}
int modsx_daisy_counters(modsx_ctx *ctx, long *out, int n) {
  NEED(ctx);
  return read_counters("modsx_daisy_counters", ctx->daisyCounters, 3, out, n);
}

int modsx_kernel_stats(modsx_ctx *ctx, double *ms, double *work, long *launches, int n) {
  NEED(ctx); NEED(ms); NEED(work); NEED(launches);
  prof_collect(ctx);
  for (int i = 0; i < n && i < K_NCLASS; i++) { ms[i] = ctx->prof.ms[i]; work[i] = ctx->prof.work[i]; launches[i] = ctx->prof.launches[i]; }
  return K_NCLASS;
}

}  // extern "C"
