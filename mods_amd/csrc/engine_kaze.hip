// engine_kaze.hip -- the "KAZE" detector branch of the reference (imagerepresentation.cpp:678-681, 1132-1152): AKAZE's
// Create_Nonlinear_Scale_Space and Feature_Detection on the view / 255, on the GPU (kernels_kaze.hip).
//   * kaze_geometry is Allocate_Memory_Evolution with fed_tau_by_process_time: host code, shared with the job tables and with
//     modsx_kaze_geometry;
//   * a call takes its images in launch sets of at most MAXB.  A set builds every stage's job records up front and sends them in one
//     copy; a stage is then one launch over the images that have the level (the two Gaussian passes go through launch_blur_pass,
//     which takes one image);
//   * the host waits four times per set: for the histograms (it walks them as compute_k_percentile does and sends back the contrast
//     factors, the only wait before the scale space), for the number of maxima, for the maxima, and for the nine Ldet values around
//     every survivor of the two filter passes;
//   * the filter passes of Find_Scale_Space_Extrema and the erase loop of Do_Subpixel_Refinement depend on the order of the list: they
//     run here on the host as the reference writes them;
//   * keypoints are filled as the branch fills det_kp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <chrono>
#include <string>
#include "engine_api.hpp"

namespace mx {

static int kz_round(float flt) { return (int)(flt + 0.5f); }      // aka::fRound

// fed_is_prime_internal (fed.cpp:158-186)
static bool kz_is_prime(int number) {
  if (number <= 1) return false;
  if (number == 2 || number == 3 || number == 5 || number == 7) return true;
  if (number % 2 == 0 || number % 3 == 0 || number % 5 == 0 || number % 7 == 0) return false;
  bool prime = true;
  const int upper = (int)sqrt(number + 1.0);
  for (int d = 11; d <= upper; d += 2)
    if (number % d == 0) prime = false;
  return prime;
}

// fed_tau_by_process_time(T, 1, 0.25, true, tau) (fed.cpp:50-150)
static std::vector<float> kz_fed_tau(float T) {
  const float tau_max = 0.25f, t = T / (float)1;
  const int n = (int)(ceil(sqrt(3.0 * t / tau_max + 0.25f) - 0.5f - 1.0e-8f) + 0.5f);
  std::vector<float> tau;
  if (n <= 0) return tau;
  const float scale = 3.0 * t / (tau_max * (float)(n * (n + 1)));
  tau.resize(n);
  std::vector<float> tauh(n);
  const float c = 1.0f / (4.0f * (float)n + 2.0f), d = scale * tau_max / 2.0f;
  for (int k = 0; k < n; ++k) {
    const float h = cos(M_PI * (2.0f * (float)k + 1.0f) * c);
    tauh[k] = d / (h * h);
  }
  const int kappa = n / 2;
  int prime = n + 1;
  while (!kz_is_prime(prime)) prime++;
  for (int k = 0, l = 0; l < n; ++k, ++l) {
    int index = 0;
    while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
    tau[l] = tauh[index];
  }
  return tau;
}

int kaze_geometry(const char *fn, int rows, int cols, const modsx_kaze_params &p, std::vector<KazeLevel> &lv, int *omax) {
  auto bad = [&](const std::string &what) { set_error(std::string(fn) + ": " + what); return MODSX_ERR_ARG; };
  if (rows < 3 || cols < 3) return bad("bad image size (at least 3 x 3)");
  if (p.diffusivity != 1)
    return bad("only the PM_G2 diffusivity (1) is built: PM_G1, WEICKERT and CHARBONNIER call OpenCV's exp / pow / sqrt, whose arithmetic is not specified");
  if (p.omax < 1 || p.omax > KZ_MAX_OCTAVES || p.nsublevels < 1 || p.omax * p.nsublevels > KZ_MAX_LEVELS)
    return bad("omax must be 1 .. 8, nsublevels at least 1, and their product at most " + std::to_string(KZ_MAX_LEVELS));
  if (!(p.soffset > 0) || !(p.soffset <= 16) || !(p.derivative_factor > 0)) return bad("soffset must be in (0, 16] and derivative_factor positive");
  if (p.kcontrast_nbins < 1 || p.kcontrast_nbins > KZ_MAX_BINS) return bad("kcontrast_nbins must be 1 .. " + std::to_string(KZ_MAX_BINS));
  if (p.descriptor < 0 || p.descriptor > 5) return bad("descriptor must be 0 .. 5");
  lv.clear();
  int om = p.omax;
  for (int i = 0; i <= p.omax - 1; i++) {
    const float rfactor = 1.0 / pow(2.f, i);
    const int h = (int)(rows * rfactor), w = (int)(cols * rfactor);
    if ((w < 80 || h < 40) && i != 0) { om = i; break; }
    for (int j = 0; j < p.nsublevels; j++) {
      KazeLevel L;
      L.esigma = p.soffset * powf(2.f, (float)(j) / (float)(p.nsublevels) + i);
      L.sigma_size = kz_round(L.esigma);
      L.etime = 0.5 * (L.esigma * L.esigma);
      L.octave = i; L.sublevel = j; L.rows = h; L.cols = w;
      const float ratio = powf(2.f, (float)i);
      L.dsize = kz_round(L.esigma * p.derivative_factor / ratio);
      L.ksize = 3 + 2 * (L.dsize - 1);
      L.nsteps = 0;
      if (L.dsize < 1 || L.dsize > KZ_MAX_S) return bad("a derivative distance of " + std::to_string(L.dsize) + " (it must be 1 .. " + std::to_string(KZ_MAX_S) + ")");
      lv.push_back(L);
    }
  }
  for (size_t i = 1; i < lv.size(); i++) {
    lv[i].tau = kz_fed_tau(lv[i].etime - lv[i - 1].etime);
    lv[i].nsteps = (int)lv[i].tau.size();
    if (lv[i].nsteps > KZ_MAX_TAU) return bad("more than " + std::to_string(KZ_MAX_TAU) + " diffusion steps in a level");
  }
  if (omax) *omax = om;
  return (int)lv.size();
}

void kaze_regions(const modsx_keypoint *kps, int n, int img_id, modsx_region *out) {
  for (int i = 0; i < n; i++) {
    modsx_region &r = out[i];
    memset(&r, 0, sizeof r);
    r.img_id = img_id; r.img_reproj_id = 0; r.type = MODSX_DET_KAZE; r.id = i;
    r.det_kp = kps[i];
  }
}

// AKAZE's size rule for a Gaussian (gaussian_2D_convolution, nldiffusion_functions.cpp:39-54)
static int kz_blur_ksize(float sigma) {
  size_t k = ceil(2.0 * (1.0 + (sigma - 0.8) / (0.3)));
  if ((k % 2) == 0) k += 1;
  return (int)k;
}

// compute_derivative_kernels' order-0 taps (nldiffusion_functions.cpp:352-394); scale 1 is getDerivKernels normalised: [3, 10, 3] / 32
static void kz_smooth_taps(int scale, float *t) {
  if (scale == 1) { t[0] = (float)(3 * (1. / 32)); t[1] = (float)(10 * (1. / 32)); t[2] = t[0]; return; }
  const float w = 10.0 / 3.0;
  const float norm = 1.0 / (2.0 * scale * (w + 2.0));
  t[0] = norm; t[1] = w * norm; t[2] = norm;
}

namespace {
struct Img {        // one image of a launch set
  int rows, cols;
  std::vector<KazeLevel> lv;
  const float *src;
  float *g, *A, *B, *sm, *flow, *lx, *ly, *tmp;
  std::vector<size_t> ldetOfs;       // of every level's plane in the Ldet arena
  size_t ldetFloats = 0;             // of all its levels
};
struct Stage { int first = 0, count = 0, blocks = 0; };
struct Builder {
  std::vector<KzJob> jobs;
  Stage begin() const { Stage s; s.first = (int)jobs.size(); return s; }
  void add(Stage &s, KzJob J, int blocks, int tilesX) { J.blk0 = s.blocks; J.tilesX = tilesX; jobs.push_back(J); s.count++; s.blocks += blocks; }
};
int tiles_stencil(int rows, int cols, int *tilesX) { *tilesX = (cols + KZ_TW - 1) / KZ_TW; return *tilesX * ((rows + KZ_TH - 1) / KZ_TH); }
int tiles_pixel(int rows, int cols, int *tilesX) { *tilesX = (cols + 63) / 64; return *tilesX * ((rows + 3) / 4); }
}  // namespace

// the two filter passes of Find_Scale_Space_Extrema (AKAZE.cpp:301-384) over the raw maxima of one image, in scan order.  The
// comparisons, their operands and their order are the reference's; what is left out changes no outcome (8 382 maxima of a 1024 x 768
// view against up to 2 796 entries each were most of a call's time):
//   * the first pass reads entries of class i and i - 1 only, and the maxima come level by level, so it walks `active`, the slots
//     of those two classes in slot order (rebuilt when the level changes; a push appends the largest slot, a replacement keeps
//     its slot and turns its class into i);
//   * the second pass reads later entries of class + 1 only: it walks that class's slots behind i;
//   * an entry further away than size along one axis is skipped before its distance is formed (sqrt and the rounding to f32 are
//     monotonic, so its distance exceeds size as well)
static void kz_filter(const std::vector<KazeLevel> &lv, const modsx_kaze_params &p, const KzRaw *raw, size_t n, KazeLists &L) {
  float smax = 0.0f;
  if (p.descriptor == 0 || p.descriptor == 1 || p.descriptor == 4 || p.descriptor == 5) smax = 10.0 * sqrtf(2.0);
  else if (p.descriptor == 2 || p.descriptor == 3) smax = 12.0 * sqrtf(2.0);
  std::vector<modsx_kaze_point> &aux = L.aux;
  aux.clear(); L.upper.clear();
  std::vector<size_t> active;
  int activeLevel = -1;
  for (size_t q = 0; q < n; q++) {
    const KzRaw &e = raw[q];
    const KazeLevel &lev = lv[e.level];
    bool is_extremum = true, is_repeated = false;
    size_t id_repeated = 0;
    modsx_kaze_point point;
    point.response = fabs(e.value);
    point.size = lev.esigma * p.derivative_factor;
    point.octave = lev.octave;
    point.class_id = e.level;
    const float ratio = pow(2.f, point.octave);
    const int sigma_size_ = kz_round(point.size / ratio);
    point.x = e.c;
    point.y = e.r;
    if (e.level != activeLevel) {
      activeLevel = e.level;
      active.clear();
      for (size_t ik = 0; ik < aux.size(); ik++)
        if ((point.class_id - 1) == aux[ik].class_id || point.class_id == aux[ik].class_id) active.push_back(ik);
    }
    for (size_t ia = 0; ia < active.size(); ia++) {
      const size_t ik = active[ia];
      const float dx = point.x * ratio - aux[ik].x, dy = point.y * ratio - aux[ik].y;
      if (fabsf(dx) > point.size || fabsf(dy) > point.size) continue;
      const float dist = sqrt(pow((double)dx, 2) + pow((double)dy, 2));
      if (dist <= point.size) {
        if (point.response > aux[ik].response) { id_repeated = ik; is_repeated = true; }
        else is_extremum = false;
        break;
      }
    }
    if (!is_extremum) continue;
    const int left_x = kz_round(point.x - smax * sigma_size_) - 1, right_x = kz_round(point.x + smax * sigma_size_) + 1;
    const int up_y = kz_round(point.y - smax * sigma_size_) - 1, down_y = kz_round(point.y + smax * sigma_size_) + 1;
    if (left_x < 0 || right_x >= lev.cols || up_y < 0 || down_y >= lev.rows) continue;
    point.x *= ratio;
    point.y *= ratio;
    if (!is_repeated) { active.push_back(aux.size()); aux.push_back(point); } else aux[id_repeated] = point;
  }
  std::vector<std::vector<size_t>> byClass(lv.size() + 1);
  for (size_t i = 0; i < aux.size(); i++) byClass[aux[i].class_id].push_back(i);
  for (size_t i = 0; i < aux.size(); i++) {
    bool is_repeated = false;
    const modsx_kaze_point &point = aux[i];
    const std::vector<size_t> &up = byClass[point.class_id + 1];
    for (size_t ju = std::upper_bound(up.begin(), up.end(), i) - up.begin(); ju < up.size(); ju++) {
      const size_t j = up[ju];
      const float dx = point.x - aux[j].x, dy = point.y - aux[j].y;
      if (fabsf(dx) > point.size || fabsf(dy) > point.size) continue;
      const float dist = sqrt(pow((double)dx, 2) + pow((double)dy, 2));
      if (dist <= point.size && point.response < aux[j].response) { is_repeated = true; break; }
    }
    if (!is_repeated) L.upper.push_back(point);
  }
}

// Do_Subpixel_Refinement (AKAZE.cpp:395-460) of the upper list; nine [k][9]: the Ldet values around (y, x) of point k, rows top to
// bottom.  cv::solve is the 2 x 2 rule of modsx.h
static void kz_refine(const std::vector<KazeLevel> &lv, const float *nine, KazeLists &L) {
  float dst[2] = {0.0f, 0.0f};
  L.final.clear();
  for (size_t i = 0; i < L.upper.size(); i++) {
    modsx_kaze_point kp = L.upper[i];
    const float *v = nine + 9 * i;
    const float ratio = pow(2.f, kp.octave);
    const int x = kz_round(kp.x / ratio), y = kz_round(kp.y / ratio);
    const float Dx = (0.5) * (v[5] - v[3]), Dy = (0.5) * (v[7] - v[1]);
    const float Dxx = (v[5] + v[3] - 2.0 * v[4]), Dyy = (v[7] + v[1] - 2.0 * v[4]);
    const float Dxy = (0.25) * (v[8] + v[0]) - (0.25) * (v[2] + v[6]);
    const float a00 = Dxx, a01 = Dxy, a10 = Dxy, a11 = Dyy, b0 = -Dx, b1 = -Dy;
    double d = (double)a00 * a11 - (double)a01 * a10;
    if (d != 0.) {
      d = 1. / d;
      const double t = ((double)b0 * a11 - (double)b1 * a01) * d;
      dst[1] = (float)(((double)b1 * a00 - (double)b0 * a10) * d);
      dst[0] = (float)t;
    }
    if (fabs(dst[0]) <= 1.0 && fabs(dst[1]) <= 1.0) {
      kp.x = x + dst[0];
      kp.y = y + dst[1];
      kp.x *= powf(2.f, lv[kp.class_id].octave);
      kp.y *= powf(2.f, lv[kp.class_id].octave);
      kp.size *= 2.0;
      L.final.push_back(kp);
    }
  }
}

static size_t align4(size_t floats) { return (floats + 3) & ~(size_t)3; }

// the geometry of a set's images, their planes in the Ldet arena (kzLdet is sized here)
static int kz_images(modsx_ctx *c, const char *fn, const int *rows, const int *cols, int n, const modsx_kaze_params &p, std::vector<Img> &im) {
  im.resize(n);
  size_t total = 0;
  for (int j = 0; j < n; j++) {
    Img &I = im[j];
    I.rows = rows[j]; I.cols = cols[j];
    const int nl = kaze_geometry(fn, rows[j], cols[j], p, I.lv, nullptr);
    if (nl < 0) return nl;
    I.ldetFloats = 0;
    for (const KazeLevel &L : I.lv) { I.ldetOfs.push_back(total + I.ldetFloats); I.ldetFloats += align4((size_t)L.rows * L.cols); }
    total += I.ldetFloats;
  }
  if (!c->kzLdet.ensure(total * 4 + 16)) return MODSX_ERR_NOMEM;
  return MODSX_OK;
}

// the scan of the Ldet planes the arena holds, the filter passes, the gather and the refinement: lists [n]
static int kz_scan(modsx_ctx *c, const std::vector<Img> &im, const modsx_kaze_params &p, std::vector<KazeLists> &lists) {
  const int n = (int)im.size();
  const float *ldet = (const float *)c->kzLdet.p;
  std::vector<KzJob> jobs;
  std::vector<int> tile0;
  int tiles = 0;
  for (int j = 0; j < n; j++) {
    tile0.push_back(tiles);
    for (size_t i = 0; i < im[j].lv.size(); i++) {
      KzJob J = {};
      J.in0 = ldet + im[j].ldetOfs[i]; J.rows = im[j].lv[i].rows; J.cols = im[j].lv[i].cols; J.slot = j; J.level = (int)i;
      J.octave = im[j].lv[i].octave; J.blk0 = tiles;
      tiles += (int)(((size_t)J.rows * J.cols + KZ_TILE - 1) / KZ_TILE);
      jobs.push_back(J);
    }
  }
  tile0.push_back(tiles);
  size_t o = 0;
  auto place = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 16); return at; };
  const size_t oJobs = place(sizeof(KzJob) * jobs.size()), oTile0 = place(sizeof(int) * tile0.size()), hostBytes = o,
               oStart = place(sizeof(int) * (n + 1)), oOffs = place(sizeof(int) * ((size_t)tiles + 1));
  if (!c->kzHost.ensure(hostBytes) || !c->kzTab.ensure(o) || !c->kzFlags.ensure((size_t)tiles * KZ_TILE + 1) ||
      !c->kzCounts.ensure((size_t)tiles * 4 + 4) || !c->kzBack.ensure(sizeof(int) * (n + 1)))
    return MODSX_ERR_NOMEM;
  char *h = (char *)c->kzHost.p, *d = (char *)c->kzTab.p;
  memcpy(h + oJobs, jobs.data(), sizeof(KzJob) * jobs.size());
  memcpy(h + oTile0, tile0.data(), sizeof(int) * tile0.size());
  MX_HIP(hipMemcpyAsync(d, h, hostBytes, hipMemcpyHostToDevice, c->stream));
  const KzJob *dJobs = (const KzJob *)(d + oJobs);
  int *offs = (int *)(d + oOffs);
  launch_kaze_scan(c->stream, dJobs, (int)jobs.size(), tiles, p.dthreshold, p.min_dthreshold, (unsigned char *)c->kzFlags.p,
                   (int *)c->kzCounts.p, offs, (const int *)(d + oTile0), n, (int *)(d + oStart));
  MX_HIP(hipMemcpyAsync(c->kzBack.p, d + oStart, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  c->kzCounters[2] += 2; c->kzCounters[4]++;
  std::vector<int> start((const int *)c->kzBack.p, (const int *)c->kzBack.p + n + 1);
  const size_t nRaw = (size_t)start[n];
  std::vector<KzRaw> raw(nRaw);
  if (nRaw) {
    if (!c->kzRaw.ensure(nRaw * sizeof(KzRaw))) return MODSX_ERR_NOMEM;
    launch_kaze_emit(c->stream, dJobs, (int)jobs.size(), tiles, (const unsigned char *)c->kzFlags.p, offs, (KzRaw *)c->kzRaw.p,
                     (int)std::min<size_t>(nRaw, 0x7fffffff));
    MX_HIP(hipMemcpyAsync(raw.data(), c->kzRaw.p, nRaw * sizeof(KzRaw), hipMemcpyDeviceToHost, c->stream));
    MX_HIP(hipStreamSynchronize(c->stream));
    MX_HIP(hipGetLastError());
    c->kzCounters[2]++; c->kzCounters[4]++;
  }
  lists.assign(n, KazeLists());
  std::vector<KzItem> items;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b2) {
    return (long)std::chrono::duration_cast<std::chrono::microseconds>(b2 - a).count();
  };
  const auto tFilter = now();
  for (int j = 0; j < n; j++) {
    KazeLists &L = lists[j];
    for (int k = start[j]; k < start[j + 1]; k++) {
      L.raw.push_back(raw[k].level); L.raw.push_back(raw[k].r); L.raw.push_back(raw[k].c);
      L.rawv.push_back(raw[k].value);
    }
    kz_filter(im[j].lv, p, raw.data() + start[j], (size_t)(start[j + 1] - start[j]), L);
    for (const modsx_kaze_point &kp : L.upper) {
      const float ratio = pow(2.f, kp.octave);
      KzItem it;
      it.ofs = im[j].ldetOfs[kp.class_id]; it.cols = im[j].lv[kp.class_id].cols;
      it.x = kz_round(kp.x / ratio); it.y = kz_round(kp.y / ratio); it.pad = 0;
      items.push_back(it);
    }
  }
  c->kzCounters[8] += us(tFilter, now());
  std::vector<float> nine(items.size() * 9);
  if (!items.empty()) {
    if (!c->kzItems.ensure(items.size() * sizeof(KzItem)) || !c->kzNine.ensure(nine.size() * 4)) return MODSX_ERR_NOMEM;
    MX_HIP(hipMemcpyAsync(c->kzItems.p, items.data(), items.size() * sizeof(KzItem), hipMemcpyHostToDevice, c->stream));
    launch_kaze_gather(c->stream, (const KzItem *)c->kzItems.p, (int)items.size(), ldet, (float *)c->kzNine.p);
    MX_HIP(hipMemcpyAsync(nine.data(), c->kzNine.p, nine.size() * 4, hipMemcpyDeviceToHost, c->stream));
    MX_HIP(hipStreamSynchronize(c->stream));
    MX_HIP(hipGetLastError());
    c->kzCounters[2]++; c->kzCounters[4]++;
  }
  size_t at = 0;
  const auto tRefine = now();
  for (int j = 0; j < n; j++) {
    kz_refine(im[j].lv, nine.data() + 9 * at, lists[j]);
    at += lists[j].upper.size();
    c->kzCounters[5] += (long)lists[j].rawv.size(); c->kzCounters[6] += (long)lists[j].upper.size(); c->kzCounters[7] += (long)lists[j].final.size();
  }
  c->kzCounters[8] += us(tRefine, now());
  return MODSX_OK;
}

// compute_k_percentile's walk (nldiffusion_functions.cpp:214-229) over integer counts: its float counters stop growing at 2^24
static float kz_walk(const unsigned *bins, int nbins, float hmax, float perc) {
  const unsigned cap = 1u << 24;
  unsigned long long total = 0;
  for (int k = 0; k < nbins; k++) total += bins[k];
  const float npoints = (float)std::min<unsigned long long>(total, cap);
  const size_t nthreshold = (size_t)(npoints * perc);
  size_t nelements = 0, k = 0;
  for (k = 0; nelements < nthreshold && k < (size_t)nbins; k++) nelements = nelements + (float)std::min(bins[k], cap);
  if (nelements < nthreshold) return 0.03;
  return hmax * ((float)(k) / (float)nbins);
}

static int run_set(modsx_ctx *c, const char *fn, const modsx_image *const *imgs, int n, const modsx_kaze_params &p,
                   std::vector<modsx_keypoint> *out, const KazeTap *tap) {
  std::vector<Img> im;
  std::vector<int> rows(n), cols(n);
  for (int j = 0; j < n; j++) { rows[j] = imgs[j]->rows; cols[j] = imgs[j]->cols; }
  int rc = kz_images(c, fn, rows.data(), cols.data(), n, p, im);
  if (rc) return rc;
  float *ldet = (float *)c->kzLdet.p;
  const int nbins = p.kcontrast_nbins;
  // the scratch planes: per image the scaled view, Lt twice, Lsmooth, Lflow, Lx, Ly and the blur's row pass, each of level 0's size
  size_t planeFloats = 0;
  size_t maxLevels = 0;
  for (Img &I : im) planeFloats += 8 * align4((size_t)I.rows * I.cols), maxLevels = std::max(maxLevels, I.lv.size());
  if (!c->kzPlanes.ensure(planeFloats * 4 + 16) || !c->kzHist.ensure((size_t)n * (nbins + 1) * 4 + (size_t)n * KZ_MAX_OCTAVES * 4 + 16) ||
      !c->kzBack.ensure((size_t)n * (nbins + 1) * 4))
    return MODSX_ERR_NOMEM;
  {
    float *at = (float *)c->kzPlanes.p;
    for (int j = 0; j < n; j++) {
      Img &I = im[j];
      const size_t px = align4((size_t)I.rows * I.cols);
      I.src = imgs[j]->d;
      I.g = at; I.A = at + px; I.B = at + 2 * px; I.sm = at + 3 * px; I.flow = at + 4 * px; I.lx = at + 5 * px; I.ly = at + 6 * px; I.tmp = at + 7 * px;
      at += 8 * px;
    }
  }
  unsigned *hist = (unsigned *)c->kzHist.p;
  float *kinv = (float *)(hist + (size_t)n * (nbins + 1));
  // every stage's job records.  Lt lives in A or B: a half-size resize and every diffusion step write the other one
  Builder b;
  int tx;
  Stage sScale = b.begin();
  for (int j = 0; j < n; j++) {
    KzJob J = {}; J.in0 = im[j].src; J.out0 = im[j].g; J.rows = im[j].rows; J.cols = im[j].cols; J.slot = j;
    b.add(sScale, J, (int)(((size_t)J.rows * J.cols + 255) / 256), 1);
  }
  Stage sGrad = b.begin();      // the Scharr derivatives of the blurred view (in sm): the maximum and the histogram
  for (int j = 0; j < n; j++) {
    KzJob J = {}; J.in0 = im[j].sm; J.rows = im[j].rows; J.cols = im[j].cols; J.slot = j; J.s = 1; J.t0 = 3.f; J.t1 = 10.f; J.t2 = 3.f;
    const int blocks = tiles_stencil(J.rows, J.cols, &tx);
    b.add(sGrad, J, blocks, tx);
  }
  std::vector<Stage> sHalf(maxLevels), sFlow(maxLevels), sDeriv(maxLevels), sSecond(maxLevels), sFed0(maxLevels), sFed1(maxLevels);
  std::vector<char> curIsA(maxLevels, 1);      // where Lt of the level is when its blur reads it
  bool curA = true;
  auto cur = [&](const Img &I, bool a) { return a ? I.A : I.B; };
  for (size_t i = 0; i < maxLevels; i++) {
    sHalf[i] = b.begin();
    if (i > 0 && (int)(i % p.nsublevels) == 0) {
      for (int j = 0; j < n; j++) {
        if (i >= im[j].lv.size()) continue;
        KzJob J = {}; J.in0 = cur(im[j], curA); J.out0 = cur(im[j], !curA); J.rows = im[j].lv[i].rows; J.cols = im[j].lv[i].cols;
        J.srows = im[j].lv[i - 1].rows; J.scols = im[j].lv[i - 1].cols; J.slot = j;
        const int blocks = tiles_pixel(J.rows, J.cols, &tx);
        b.add(sHalf[i], J, blocks, tx);
      }
      curA = !curA;
    }
    curIsA[i] = curA;
    sFlow[i] = b.begin();
    if (i > 0)
      for (int j = 0; j < n; j++) {
        if (i >= im[j].lv.size()) continue;
        KzJob J = {}; J.in0 = im[j].sm; J.out0 = im[j].flow; J.rows = im[j].lv[i].rows; J.cols = im[j].lv[i].cols; J.slot = j;
        J.octave = im[j].lv[i].octave; J.s = 1; J.t0 = 3.f; J.t1 = 10.f; J.t2 = 3.f;
        const int blocks = tiles_stencil(J.rows, J.cols, &tx);
        b.add(sFlow[i], J, blocks, tx);
      }
    sDeriv[i] = b.begin();
    for (int j = 0; j < n; j++) {
      if (i >= im[j].lv.size()) continue;
      const KazeLevel &L = im[j].lv[i];
      KzJob J = {}; J.in0 = i == 0 ? cur(im[j], curA) : im[j].sm; J.out0 = im[j].lx; J.out1 = im[j].ly; J.rows = L.rows; J.cols = L.cols; J.slot = j;
      J.s = L.dsize;
      float t[3];
      kz_smooth_taps(L.dsize, t);
      J.t0 = t[0]; J.t1 = t[1]; J.t2 = t[2];
      const int blocks = tiles_stencil(J.rows, J.cols, &tx);
      b.add(sDeriv[i], J, blocks, tx);
    }
    sSecond[i] = b.begin();
    for (int j = 0; j < n; j++) {
      if (i >= im[j].lv.size()) continue;
      const KazeLevel &L = im[j].lv[i];
      KzJob J = {}; J.in0 = im[j].lx; J.in1 = im[j].ly; J.out0 = ldet + im[j].ldetOfs[i]; J.rows = L.rows; J.cols = L.cols; J.slot = j;
      J.s = L.dsize; J.scale = (float)(L.dsize * L.dsize);
      float t[3];
      kz_smooth_taps(L.dsize, t);
      J.t0 = t[0]; J.t1 = t[1]; J.t2 = t[2];
      const int blocks = tiles_stencil(J.rows, J.cols, &tx);
      b.add(sSecond[i], J, blocks, tx);
    }
    sFed0[i] = b.begin();
    for (int j = 0; j < n && i > 0; j++) {
      if (i >= im[j].lv.size()) continue;
      KzJob J = {}; J.in0 = cur(im[j], curA); J.in1 = im[j].flow; J.out0 = cur(im[j], !curA); J.rows = im[j].lv[i].rows; J.cols = im[j].lv[i].cols; J.slot = j;
      const int blocks = tiles_pixel(J.rows, J.cols, &tx);
      b.add(sFed0[i], J, blocks, tx);
    }
    sFed1[i] = b.begin();
    for (int j = 0; j < n && i > 0; j++) {
      if (i >= im[j].lv.size()) continue;
      KzJob J = {}; J.in0 = cur(im[j], !curA); J.in1 = im[j].flow; J.out0 = cur(im[j], curA); J.rows = im[j].lv[i].rows; J.cols = im[j].lv[i].cols; J.slot = j;
      const int blocks = tiles_pixel(J.rows, J.cols, &tx);
      b.add(sFed1[i], J, blocks, tx);
    }
    // the steps of a level are the same for every image: the level table depends on the image through its size alone
    int nsteps = 0;
    for (int j = 0; j < n; j++) if (i < im[j].lv.size()) nsteps = im[j].lv[i].nsteps;
    if (nsteps & 1) curA = !curA;
  }
  // one copy: the job records, then the taps of the two Gaussians
  const int n1 = kz_blur_ksize(1.0f), n0 = kz_blur_ksize(p.soffset);
  const std::vector<float> g1 = gaussian_kernel(n1, 1.0), g0 = gaussian_kernel(n0, (double)p.soffset);
  size_t o = 0;
  auto place = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 16); return at; };
  const size_t oJobs = place(sizeof(KzJob) * b.jobs.size()), oG1 = place(4 * (size_t)n1), oG0 = place(4 * (size_t)n0);
  if (!c->kzHost.ensure(o) || !c->kzTab.ensure(o)) return MODSX_ERR_NOMEM;
  char *h = (char *)c->kzHost.p, *d = (char *)c->kzTab.p;
  memcpy(h + oJobs, b.jobs.data(), sizeof(KzJob) * b.jobs.size());
  memcpy(h + oG1, g1.data(), 4 * (size_t)n1);
  memcpy(h + oG0, g0.data(), 4 * (size_t)n0);
  hipStream_t s = c->stream;
  MX_HIP(hipMemcpyAsync(d, h, o, hipMemcpyHostToDevice, s));
  MX_HIP(hipMemsetAsync(hist, 0, (size_t)n * (nbins + 1) * 4, s));
  const KzJob *dj = (const KzJob *)(d + oJobs);
  const float *dG1 = (const float *)(d + oG1), *dG0 = (const float *)(d + oG0);
  long launches = 0;
  auto blur = [&](const Img &I, const float *src, float *dst, int rws, int cls, const float *taps, int nt) {
    launch_blur_pass(s, src, I.tmp, rws, cls, taps, nt, 0, 1);
    launch_blur_pass(s, I.tmp, dst, rws, cls, taps, nt, 1, 1);
    launches += 2;
  };
  // the contrast factor: the gradient histogram of the view blurred with sigma 1
  launch_kaze_scale(s, dj + sScale.first, sScale.count, sScale.blocks);
  for (const Img &I : im) blur(I, I.g, I.sm, I.rows, I.cols, dG1, n1);
  launch_kaze_first(s, KZ_MAX, dj + sGrad.first, sGrad.count, sGrad.blocks, kinv, hist, nbins);
  launch_kaze_first(s, KZ_HIST, dj + sGrad.first, sGrad.count, sGrad.blocks, kinv, hist, nbins);
  launches += 3;
  MX_HIP(hipMemcpyAsync(c->kzBack.p, hist, (size_t)n * (nbins + 1) * 4, hipMemcpyDeviceToHost, s));
  MX_HIP(hipStreamSynchronize(s));
  MX_HIP(hipGetLastError());
  c->kzCounters[4]++;
  std::vector<float> hostKinv((size_t)n * KZ_MAX_OCTAVES, 0.f);
  for (int j = 0; j < n; j++) {
    const unsigned *hj = (const unsigned *)c->kzBack.p + (size_t)j * (nbins + 1);
    float hmax;
    memcpy(&hmax, hj, 4);
    const float k0 = kz_walk(hj + 1, nbins, hmax, p.kcontrast_percentile);
    float kc = k0;
    for (int oc = 0; oc < KZ_MAX_OCTAVES; oc++) {
      hostKinv[(size_t)j * KZ_MAX_OCTAVES + oc] = (float)(1.0 / (double)(kc * kc));
      kc = kc * 0.75;
    }
    if (tap) {
      tap->kc[0] = k0; tap->kc[1] = hmax;
      for (int k = 0; k < nbins; k++) tap->hist[k] = (long)hj[1 + k];
    }
  }
  MX_HIP(hipMemcpyAsync(kinv, hostKinv.data(), hostKinv.size() * 4, hipMemcpyHostToDevice, s));
  // the scale space, level by level
  size_t tapOfs = 0;
  curA = true;
  for (const Img &I : im) blur(I, I.g, I.A, I.rows, I.cols, dG0, n0);
  for (size_t i = 0; i < maxLevels; i++) {
    if (sHalf[i].count) { launch_kaze_half(s, dj + sHalf[i].first, sHalf[i].count, sHalf[i].blocks); launches++; curA = !curA; }
    if (i > 0) {
      for (const Img &I : im)
        if (i < I.lv.size()) blur(I, cur(I, curA), I.sm, I.lv[i].rows, I.lv[i].cols, dG1, n1);
      launch_kaze_first(s, KZ_FLOW, dj + sFlow[i].first, sFlow[i].count, sFlow[i].blocks, kinv, hist, nbins);
      launches++;
    }
    launch_kaze_first(s, KZ_DERIV, dj + sDeriv[i].first, sDeriv[i].count, sDeriv[i].blocks, kinv, hist, nbins);
    launch_kaze_second(s, dj + sSecond[i].first, sSecond[i].count, sSecond[i].blocks);
    launches += 2;
    const std::vector<float> *tau = nullptr;
    for (const Img &I : im) if (i < I.lv.size()) tau = &I.lv[i].tau;
    for (size_t k = 0; tau && k < tau->size(); k++) {
      const Stage &st = (k & 1) ? sFed1[i] : sFed0[i];
      launch_kaze_fed(s, dj + st.first, st.count, st.blocks, (*tau)[k]);
      launches++; c->kzCounters[3]++;
    }
    if (tau && (tau->size() & 1)) curA = !curA;
    if (tap) {      // one image
      const Img &I = im[0];
      const size_t px = (size_t)I.lv[i].rows * I.lv[i].cols;
      MX_HIP(hipMemcpyAsync(tap->Lt + tapOfs, cur(I, curA), px * 4, hipMemcpyDeviceToHost, s));
      MX_HIP(hipMemcpyAsync(tap->Lsmooth + tapOfs, i == 0 ? cur(I, curA) : I.sm, px * 4, hipMemcpyDeviceToHost, s));
      if (i == 0) memset(tap->Lflow, 0, px * 4);
      else MX_HIP(hipMemcpyAsync(tap->Lflow + tapOfs, I.flow, px * 4, hipMemcpyDeviceToHost, s));
      MX_HIP(hipMemcpyAsync(tap->Ldet + tapOfs, ldet + I.ldetOfs[i], px * 4, hipMemcpyDeviceToHost, s));
      MX_HIP(hipStreamSynchronize(s));
      tapOfs += px;
    }
  }
  c->kzCounters[1] += n; c->kzCounters[2] += launches;
  std::vector<KazeLists> lists;
  if ((rc = kz_scan(c, im, p, lists))) return rc;
  if (out)
    for (int j = 0; j < n; j++) {
      out[j].clear();
      for (const modsx_kaze_point &q : lists[j].final) {
        modsx_keypoint kp;
        memset(&kp, 0, sizeof kp);       // the padding too: callers compare records as bytes
        kp.x = q.x; kp.y = q.y; kp.s = q.size / 3.0; kp.response = q.response;
        kp.a11 = cos(0.0); kp.a12 = sin(0.0); kp.a21 = -sin(0.0); kp.a22 = cos(0.0);
        kp.octave_number = q.octave;
        out[j].push_back(kp);
      }
    }
  if (tap) *tap->lists = lists[0];
  return MODSX_OK;
}

static int kz_check(const char *fn, const modsx_image *const *imgs, int n, const modsx_kaze_params &p) {
  for (int i = 0; i < n; i++) {
    if (!imgs[i] || !imgs[i]->d) { set_error(std::string(fn) + ": null image"); return MODSX_ERR_ARG; }
    std::vector<KazeLevel> lv;
    const int rc = kaze_geometry(fn, imgs[i]->rows, imgs[i]->cols, p, lv, nullptr);
    if (rc < 0) return rc;
  }
  return MODSX_OK;
}

int detect_kaze_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_kaze_params &par, std::vector<modsx_keypoint> *out) {
  int rc = kz_check("modsx_detect_kaze", imgs, n, par);
  if (rc) return rc;
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  c->kzCounters[0]++;
  for (int i0 = 0; i0 < n; i0 += MAXB)
    if ((rc = run_set(c, "modsx_detect_kaze", imgs + i0, std::min(MAXB, n - i0), par, out + i0, nullptr))) return rc;
  return MODSX_OK;
}

int debug_kaze(modsx_ctx *c, const modsx_image *img, const modsx_kaze_params &par, const KazeTap &tap) {
  const modsx_image *imgs[1] = {img};
  int rc = kz_check("modsx_debug_kaze", imgs, 1, par);
  if (rc) return rc;
  CtxBusy busy(c);
  c->kzCounters[0]++;
  if ((rc = run_set(c, "modsx_debug_kaze", imgs, 1, par, nullptr, &tap))) return rc;
  std::vector<KazeLevel> lv;
  return kaze_geometry("modsx_debug_kaze", img->rows, img->cols, par, lv, nullptr);
}

int debug_kaze_scan(modsx_ctx *c, int rows, int cols, const modsx_kaze_params &par, const float *ldet, KazeLists &lists) {
  std::vector<Img> im;
  int rc = kz_images(c, "modsx_debug_kaze_scan", &rows, &cols, 1, par, im);
  if (rc) return rc;
  CtxBusy busy(c);
  c->kzCounters[0]++; c->kzCounters[1]++;
  size_t at = 0;
  for (size_t i = 0; i < im[0].lv.size(); i++) {
    const size_t px = (size_t)im[0].lv[i].rows * im[0].lv[i].cols;
    MX_HIP(hipMemcpyAsync((float *)c->kzLdet.p + im[0].ldetOfs[i], ldet + at, px * 4, hipMemcpyHostToDevice, c->stream));
    at += px;
  }
  std::vector<KazeLists> all;
  if ((rc = kz_scan(c, im, par, all))) return rc;
  lists = all[0];
  return (int)im[0].lv.size();
}

}  // namespace mx
