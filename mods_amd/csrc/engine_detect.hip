// engine_detect.hip -- the detection front end of the device path: scale-space pyramid, extrema scan, detection order,
// affine adaptation and the export rules (ScaleSpaceDetector / AffineDetector of the reference).  Context, waits, copies and the
// later stages (orientation, description, matching, verification) are in engine.hip.
#include <math.h>
#include <algorithm>
#include <mutex>
#include <dlfcn.h>
#include <string>
#include "engine_api.hpp"

namespace mx {

// ------------------------------------------------------------------------------------------------
// pyramid
// ------------------------------------------------------------------------------------------------
static int cv_round(double v) { return (int)lrint(v); }  // cvRound: round half to even

struct SigmaPlan {
  int levels;
  float sigmaStep;
  float curSigma[8];   // sigma of level i (pyramid.cpp:458-459, 532)
  float incSigma[8];   // blur applied to level i-1 to get level i (:483)
};

static SigmaPlan make_sigma_plan(const modsx_hessaff_params &p) {
  SigmaPlan s;
  s.levels = p.numberOfScales + 2;
  s.sigmaStep = powf(2.0f, 1.0f / (float)p.numberOfScales);
  float cur = p.initialSigma;
  s.curSigma[0] = cur; s.incSigma[0] = 0;
  for (int i = 1; i < s.levels; i++) {
    s.incSigma[i] = cur * sqrtf(s.sigmaStep * s.sigmaStep - 1.0f);
    cur *= s.sigmaStep;
    s.curSigma[i] = cur;
  }
  return s;
}

static int fill_taps(BlurBatch &b, float sigma) {
  int n = blur_ksize(sigma);
  if (n > MAX_TAPS) { set_error("pyramid blur kernel larger than 17 taps is not supported"); return MODSX_ERR_ARG; }
  std::vector<float> k = gaussian_kernel(n, sigma);
  b.n = n;
  for (int i = 0; i < n; i++) b.k[i] = k[i];
  return MODSX_OK;
}

// Octave geometry of every image (pyramid.cpp:455-573) and the slab pointers of its levels in Pyramid::store
static int plan_octaves(modsx_ctx *c, const modsx_image *const *imgs, int n, int L, int minSize, bool singleOctave, int *maxOct) {
  *maxOct = 0;
  for (int i = 0; i < n; i++) {
    Pyramid &py = c->pyr[i];
    py.nOct = 0;
    int rows = imgs[i]->rows, cols = imgs[i]->cols;
    float pd = 1.0f;
    size_t total = 0;
    while (rows > minSize && cols > minSize && py.nOct < 24) {
      Octave &o = py.oct[py.nOct++];
      o.rows = rows; o.cols = cols; o.pixelDistance = pd;
      total += (size_t)2 * L * rows * cols;
      pd *= 2.0;
      rows = cv_round(rows * 0.5); cols = cv_round(cols * 0.5);
      if (singleOctave) break;
    }
    if (!py.store.ensure(total * sizeof(float) + 64)) return MODSX_ERR_NOMEM;
    float *ptr = (float *)py.store.p;
    for (int o = 0; o < py.nOct; o++) {
      size_t npx = (size_t)py.oct[o].rows * py.oct[o].cols;
      for (int l = 0; l < L; l++) { py.oct[o].blur[l] = ptr; ptr += npx; }
      for (int l = 0; l < L; l++) { py.oct[o].resp[l] = ptr; ptr += npx; }
    }
    *maxOct = std::max(*maxOct, py.nOct);
  }
  return MODSX_OK;
}

// The images of the batch that have octave o, in batch order: the jobs of every launch of that octave.  mr x mc: the largest
// of these octaves (the launches' tile grid); px: their pixels together.
struct LiveOctave {
  int n = 0, img[MAXB], mr = 0, mc = 0;
  double px = 0;
};
static LiveOctave live_octave(const modsx_ctx *c, int n, int o) {
  LiveOctave lv;
  for (int i = 0; i < n; i++) {
    if (c->pyr[i].nOct <= o) continue;
    const Octave &oc = c->pyr[i].oct[o];
    lv.img[lv.n++] = i;
    lv.mr = std::max(lv.mr, oc.rows); lv.mc = std::max(lv.mc, oc.cols);
    lv.px += (double)oc.rows * oc.cols;
  }
  return lv;
}

// Level 0 of octave 0: the image itself or, when initialSigma asks for more than the image's assumed 0.5, its blur; with the
// Hessian of the level from the same launch
static int launch_first_level(modsx_ctx *c, const modsx_image *const *imgs, const LiveOctave &lv, const modsx_hessaff_params &p,
                              const SigmaPlan &sp, bool hess, bool firstLevelGiven) {
  hipStream_t s = c->stream;
  BlurBatch bb;
  memset(&bb, 0, sizeof bb);
  const float curSigma0 = 0.5f;
  const bool preBlur = !firstLevelGiven && p.initialSigma > curSigma0;
  if (preBlur) {
    float sigma = sqrtf(p.initialSigma * p.initialSigma - curSigma0 * curSigma0);
    int rc = fill_taps(bb, sigma);
    if (rc) return rc;
  }
  for (int k = 0; k < lv.n; k++) {
    const int i = lv.img[k];
    Octave &oc = c->pyr[i].oct[0];
    BlurJob &j = bb.j[k];
    j.src = imgs[i]->d; j.blur = oc.blur[0]; j.resp = hess ? oc.resp[0] : nullptr; j.rows = oc.rows; j.cols = oc.cols;
    j.norm = sp.curSigma[0] * sp.curSigma[0];
    if (!preBlur) {
      MX_HIP(hipMemcpyAsync(oc.blur[0], imgs[i]->d, (size_t)oc.rows * oc.cols * 4, hipMemcpyDeviceToDevice, s));
      j.src = oc.blur[0];
    }
  }
  if (preBlur) { ProfScope ps(c, K_BLUR_HESS, lv.px * 12); book_blur(c, launch_blur_hess(s, bb, lv.n, lv.mr, lv.mc)); }
  else if (hess) { ProfScope ps(c, K_HESSIAN, lv.px * 8); c->detCnt[DT_HESSIAN] += launch_hessian(s, bb, lv.n, lv.mr, lv.mc); }
  return MODSX_OK;
}

// Level 0 of octave o > 0: the seed level of the octave below at half the size, with the Hessian of the new level from the same launch
static void launch_resize_level(modsx_ctx *c, const LiveOctave &lv, int o, const modsx_hessaff_params &p, const SigmaPlan &sp, bool hess) {
  ResizeBatch rb;
  memset(&rb, 0, sizeof rb);
  double spx = 0;
  for (int k = 0; k < lv.n; k++) {
    Octave &pv = c->pyr[lv.img[k]].oct[o - 1], &oc = c->pyr[lv.img[k]].oct[o];
    ResizeJob &r = rb.j[k];
    r.src = pv.blur[p.numberOfScales]; r.dst = oc.blur[0];
    r.srows = pv.rows; r.scols = pv.cols; r.drows = oc.rows; r.dcols = oc.cols;
    r.resp = hess ? oc.resp[0] : nullptr; r.norm = sp.curSigma[0] * sp.curSigma[0];
    spx += (double)pv.rows * pv.cols;
  }
  ProfScope ps(c, K_RESIZE, (spx + lv.px) * 4 + lv.px * 4);
  c->detCnt[DT_RESIZE] += launch_resize_half(c->stream, rb, lv.n, lv.mr, lv.mc);
}

// DoG / Harris (ScaleSpaceDetector::dogResponse :176-181, HarrisResponse :283-305; norm = sigma^2 of the level, :475,490):
// the response of every level of octave o from its blur, with the generic any-sigma filter passes (the DoG of a level is the level
// minus its blur with sigma = norm; Harris blurs three gradient products with sqrt(0.6 norm)) -- separate launches per image and
// level: these detectors are on no shipped configuration's path, the Hessian's fused kernels are untouched
static int launch_other_responses(modsx_ctx *c, const LiveOctave &lv, int o, const modsx_hessaff_params &p, const SigmaPlan &sp) {
  hipStream_t s = c->stream;
  const int L = sp.levels;
  constexpr int RESP_TAPS = 4096;                  // most taps of one filter pass
  constexpr size_t SLICE = 2 * (RESP_TAPS + 4);    // floats of a level's slice of the staging buffers: the row taps, then the column taps
  for (int l = 0; l < L; l++) {
    const float norm = sp.curSigma[l] * sp.curSigma[l];
    const float sigma = p.detectorType == MODSX_DET_DOG ? norm : sqrtf((float)(0.6 * norm));
    const int nt = blur_ksize(sigma);
    if (nt > RESP_TAPS) { set_error("response blur kernel too large"); return MODSX_ERR_ARG; }
    if (!c->viewTaps.ensure((size_t)L * SLICE * 4) || !c->hViewTaps.ensure((size_t)L * SLICE * 4)) return MODSX_ERR_NOMEM;
    // one slice of the staging buffers per level, so that no upload overwrites taps a queued launch still reads
    float *dT = (float *)c->viewTaps.p + (size_t)l * SLICE, *hT = (float *)c->hViewTaps.p + (size_t)l * SLICE;
    bool tapsUp = false;
    for (int k = 0; k < lv.n; k++) {
      Octave &oc = c->pyr[lv.img[k]].oct[o];
      const int rows = oc.rows, cols = oc.cols;
      const size_t npx = (size_t)rows * cols;
      if (!c->scratchA.ensure(npx * 4 * 8)) return MODSX_ERR_NOMEM;
      float *buf = (float *)c->scratchA.p, *tmp = buf, *a = buf + npx, *b = buf + 2 * npx, *cc = buf + 3 * npx;
      float *ba = buf + 4 * npx, *bb2 = buf + 5 * npx, *bc = buf + 6 * npx;
      const int nx = cols == 1 ? 1 : nt, ny = rows == 1 ? 1 : nt;
      if (!tapsUp || nx != nt || ny != nt) {
        std::vector<float> kx = gaussian_kernel(nx, sigma), ky = gaussian_kernel(ny, sigma);
        if (tapsUp) MX_HIP(ctx_sync(c));      // a degenerate (one-row / one-column) level re-uses the slice
        memcpy(hT, kx.data(), nx * 4); memcpy(hT + nx, ky.data(), ny * 4);
        MX_HIP(ctx_copy(c, dT, hT, (size_t)(nx + ny) * 4, hipMemcpyHostToDevice));
        tapsUp = nx == nt && ny == nt;
      }
      auto blur = [&](const float *src, float *dst) {
        if (nt == 1) { MX_HIP(hipMemcpyAsync(dst, src, npx * 4, hipMemcpyDeviceToDevice, s)); return MODSX_OK; }
        launch_blur_pass(s, src, tmp, rows, cols, dT, nx, 0, 1);
        launch_blur_pass(s, tmp, dst, rows, cols, dT + nx, ny, 1, 1);
        return MODSX_OK;
      };
      if (p.detectorType == MODSX_DET_DOG) {
        int rc = blur(oc.blur[l], a);
        if (rc) return rc;
        launch_sub(s, oc.blur[l], a, oc.resp[l], npx);
      } else {
        launch_grad_products(s, oc.blur[l], rows, cols, a, b, cc);
        int rc = blur(a, ba);
        if (!rc) rc = blur(b, bb2);
        if (!rc) rc = blur(cc, bc);
        if (rc) return rc;
        launch_harris_combine(s, ba, bb2, bc, (float)(0.6 * norm), oc.resp[l], npx);
      }
    }
  }
  return MODSX_OK;
}

// ScaleSpaceDetector::detectPyramidKeypoints / detectOctaveKeypoints (pyramid.cpp:455-573) for a batch
// of images: builds every blur and response level in HBM.  firstLevelGiven: the image IS the first level
// of a single octave (stage tap used by modsx_octave_levels).
int build_pyramids(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_hessaff_params &p,
                   bool singleOctaveFromFirstLevel) {
  if (n <= 0 || n > MAXB) { set_error("batch size"); return MODSX_ERR_ARG; }
  if (p.numberOfScales < 1 || p.numberOfScales > 6) { set_error("numberOfScales"); return MODSX_ERR_ARG; }
  // the scan reads rows r - 1 .. r + 1 of [border, rows - border): border 0 starts at row -1, a negative one before the plane
  // (localizeKeypoint itself reads out of bounds there, so there is no reference result either)
  if (p.border < 1) { set_error("border must be at least 1"); return MODSX_ERR_ARG; }
  if (p.detectorType != MODSX_DET_HESSIAN && p.detectorType != MODSX_DET_DOG && p.detectorType != MODSX_DET_HARRIS) {
    set_error("detectorType must be Hessian (0), DoG (1) or Harris (2)");
    return MODSX_ERR_ARG;
  }
  const bool hess = p.detectorType == MODSX_DET_HESSIAN;    // its response is fused into the blur / resize kernels; the others follow below
  const SigmaPlan sp = make_sigma_plan(p);
  int maxOct = 0;
  int rc = plan_octaves(c, imgs, n, sp.levels, 2 * p.border + 2, singleOctaveFromFirstLevel, &maxOct);
  if (rc) return rc;
  for (int o = 0; o < maxOct; o++) {
    const LiveOctave lv = live_octave(c, n, o);      // never empty: some image has maxOct octaves
    if (o == 0) rc = launch_first_level(c, imgs, lv, p, sp, hess, singleOctaveFromFirstLevel);
    else launch_resize_level(c, lv, o, p, sp, hess);
    if (rc) return rc;
    for (int l = 1; l < sp.levels; l++) {
      BlurBatch b2;
      memset(&b2, 0, sizeof b2);
      rc = fill_taps(b2, sp.incSigma[l]);
      if (rc) return rc;
      for (int k = 0; k < lv.n; k++) {
        Octave &oc = c->pyr[lv.img[k]].oct[o];
        BlurJob &j = b2.j[k];
        j.src = oc.blur[l - 1]; j.blur = oc.blur[l]; j.resp = hess ? oc.resp[l] : nullptr; j.rows = oc.rows; j.cols = oc.cols;
        j.norm = sp.curSigma[l] * sp.curSigma[l];
      }
      ProfScope ps(c, K_BLUR_HESS, lv.px * 12);
      book_blur(c, launch_blur_hess(c->stream, b2, lv.n, lv.mr, lv.mc));
    }
    if (!hess) rc = launch_other_responses(c, lv, o, p, sp);
    if (rc) return rc;
  }
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

// ------------------------------------------------------------------------------------------------
// detection: extrema + localisation on device, detection order + octaveMap + scale on host
// ------------------------------------------------------------------------------------------------
static const unsigned CAND_CAP = 1u << 21;

// thresholds, affinedetectors/pyramid.h:47-67 (DET_HESSIAN)
static NmsBatch nms_thresholds(const modsx_hessaff_params &p) {
  NmsBatch nb;
  memset(&nb, 0, sizeof nb);
  nb.edgeScoreThreshold = (p.edgeEigenValueRatio + 1.0f) * (p.edgeEigenValueRatio + 1.0f) / p.edgeEigenValueRatio;
  float finalTh = p.threshold;
  float posTh = (float)(0.8 * finalTh);
  float negTh = -posTh;
  if (p.detectorType == MODSX_DET_HESSIAN) finalTh = p.threshold * p.threshold;     // pyramid.h:56-57: squared for DET_HESSIAN only
  if (p.mode != MODSX_FIXED_TH) finalTh = posTh = negTh = 0.0f;
  nb.posTh = posTh; nb.negTh = negTh; nb.finalTh = finalTh; nb.border = p.border; nb.detType = p.detectorType;
  return nb;
}

// the context's counter block: the NMS words and sub-queue counters, then the Baumberg queue's counters
constexpr size_t COUNTER_BYTES = (NMS_QUEUES + 1) * 128 + BAUM_QUEUE_BYTES;
static unsigned *baum_queue(modsx_ctx *c) { return (unsigned *)c->counter.p + (NMS_QUEUES + 1) * 32; }
static int baum_resident(modsx_ctx *c) {   // asked once per context; 0: the runtime gave no answer
  if (!c->baumResident) { const int w = baumberg_resident_waves(); c->baumResident = w > 0 ? w : -1; }
  return c->baumResident > 0 ? c->baumResident : 0;
}

// All (image, octave, level) scans of the batch in one launch (NMS_MAXJ jobs at most per launch): the accepted candidates
// end up in c->cand, their count in word 0 of c->counter.  With the shipped numberOfScales = 3 the tiles number OCTAVES and a
// tile scans the three levels of its octave in one pass over the five response planes (k_nms_localize_oct); otherwise a tile
// belongs to one level
static int scan_extrema(modsx_ctx *c, int n, const modsx_hessaff_params &p) {
  hipStream_t s = c->stream;
  if (!c->cand.ensure((size_t)CAND_CAP * sizeof(Candidate)) || !c->nmsQueue.ensure((size_t)CAND_CAP * 16)) return MODSX_ERR_NOMEM;
  if (!c->counter.ensure(COUNTER_BYTES)) return MODSX_ERR_NOMEM;
  // [0] accepted candidates, [1] extremum-queue overflow flag, from word 32 on the sub-queue counters, behind them the counters of
  // the Baumberg queue (baum_queue: nothing before that launch writes them): one fill for the lot
  MX_HIP(hipMemsetAsync(c->counter.p, 0, COUNTER_BYTES, s));
  bool queuesClean = true;   // the sub-queue counters are zero (no scan has run since the fill)
  const NmsBatch nb = nms_thresholds(p);
  int maxOct = 0;
  for (int i = 0; i < n; i++) maxOct = std::max(maxOct, c->pyr[i].nOct);
  const bool perOctave = p.numberOfScales == 3 && !getenv("MODSX_NMS_PER_LEVEL");
  std::vector<NmsJob> hjobs;
  std::vector<int> hpfx(1, 0), hfirst;
  double px = 0;
  c->detCnt[DT_LAST_JOBS] = c->detCnt[DT_LAST_TILES] = 0;
  auto flush = [&](bool last) -> int {
    const int nj = (int)hjobs.size();
    if (!nj) return MODSX_OK;
    const int np = (int)hpfx.size() - 1;     // tile groups: octaves or levels
    const size_t jobBytes = (size_t)nj * sizeof(NmsJob), pfxBytes = (size_t)(np + 1) * 4, firstBytes = (size_t)std::max<size_t>(1, hfirst.size()) * 4;
    if (!c->nmsJobs.ensure(jobBytes + pfxBytes + firstBytes + 64)) return MODSX_ERR_NOMEM;
    if (!c->hNms.ensure(jobBytes + pfxBytes + firstBytes)) return MODSX_ERR_NOMEM;   // jobs + prefix (+ first level job of every octave): one pinned blob, one copy
    memcpy(c->hNms.p, hjobs.data(), jobBytes);
    memcpy((char *)c->hNms.p + jobBytes, hpfx.data(), pfxBytes);
    if (!hfirst.empty()) memcpy((char *)c->hNms.p + jobBytes + pfxBytes, hfirst.data(), hfirst.size() * 4);
    MX_HIP(ctx_copy(c, c->nmsJobs.p, c->hNms.p, jobBytes + pfxBytes + firstBytes, hipMemcpyHostToDevice));
    if (!c->tileJob.ensure((size_t)hpfx.back() * 4 + 4)) return MODSX_ERR_NOMEM;
    const int *dPfx = (const int *)((char *)c->nmsJobs.p + jobBytes);
    launch_expand_tiles(s, dPfx, np, (int *)c->tileJob.p);
    c->detCnt[perOctave ? DT_SCAN_OCTAVE : DT_SCAN_LEVEL]++;
    c->detCnt[DT_LAST_JOBS] += nj; c->detCnt[DT_LAST_TILES] += hpfx.back();
    if (!last) c->detCnt[DT_NMS_FLUSHES]++;     // the job table was full: a launch before the scan's last
    {
      ProfScope ps(c, K_NMS, px * 12);
      if (!queuesClean) MX_HIP(hipMemsetAsync((unsigned *)c->counter.p + 32, 0, NMS_QUEUES * 128, s));
      queuesClean = false;
      launch_nms(s, nb, (const NmsJob *)c->nmsJobs.p, dPfx, (const int *)c->tileJob.p, nj,
                 hpfx.back(), (int4 *)c->nmsQueue.p, (unsigned *)c->counter.p + 32, CAND_CAP, (Candidate *)c->cand.p,
                 (unsigned *)c->counter.p, CAND_CAP, perOctave ? (const int *)((char *)c->nmsJobs.p + jobBytes + pfxBytes) : nullptr,
                 p.numberOfScales);
    }
    // the host tables are reused by the next flush; after the last one the counter read-back waits for the launch
    if (!last) MX_HIP(ctx_sync(c));
    hjobs.clear(); hpfx.assign(1, 0); hfirst.clear(); px = 0;
    return MODSX_OK;
  };
  for (int o = 0; o < maxOct; o++)
    for (int i = 0; i < n; i++) {
      if (c->pyr[i].nOct <= o) continue;
      Octave &oc = c->pyr[i].oct[o];
      const int w = oc.cols - 2 * p.border, h = oc.rows - 2 * p.border;
      if (w <= 0 || h <= 0) continue;
      if ((int)hjobs.size() + p.numberOfScales > NMS_MAXJ) { int rcf = flush(false); if (rcf) return rcf; }
      const int tiles = ((w + 63) / 64) * ((h + NMS_TILE_ROWS - 1) / NMS_TILE_ROWS);
      if (perOctave) { hfirst.push_back((int)hjobs.size()); hpfx.push_back(hpfx.back() + tiles); }
      for (int l = 1; l <= p.numberOfScales; l++) {
        NmsJob j;
        j.low = oc.resp[l - 1]; j.cur = oc.resp[l]; j.high = oc.resp[l + 1]; j.blur = oc.blur[l];
        j.rows = oc.rows; j.cols = oc.cols; j.img = i; j.octave = o; j.level = l; j.pad = 0;
        hjobs.push_back(j);
        if (!perOctave) hpfx.push_back(hpfx.back() + tiles);
        px += (double)oc.rows * oc.cols;
      }
    }
  return flush(true);
}

// The count words of c->counter and the records of devRecords come down behind ONE wait: the records are copied speculatively,
// as many as the context's last set had (lastCount + 1/4, at most cap); a set that holds more costs a second copy of them all.
// *nrec = word recWord, the number of records.  cap is also how many candidates devRecords was made from: a set with more
// leaves only its count (c->lastCandCount), and the caller makes the records again.
static int download_counted(modsx_ctx *c, const void *devRecords, int recWord, size_t cap, size_t lastCount, unsigned *nrec) {
  if (!c->hMisc.ensure(64)) return MODSX_ERR_NOMEM;
  const size_t spec = std::min<size_t>(cap, lastCount + lastCount / 4 + 1024);
  if (!c->hCand.ensure(std::max<size_t>(spec, 1) * sizeof(Candidate))) return MODSX_ERR_NOMEM;
  MX_HIP(ctx_copy(c, c->hMisc.p, c->counter.p, std::max(2, recWord + 1) * 4, hipMemcpyDeviceToHost));
  MX_HIP(ctx_copy(c, c->hCand.p, devRecords, spec * sizeof(Candidate), hipMemcpyDeviceToHost));
  MX_HIP(ctx_sync(c));
  const unsigned *w = (const unsigned *)c->hMisc.p;
  if (w[0] > CAND_CAP || w[1]) { set_error("candidate buffer overflow"); return MODSX_ERR_NOMEM; }
  c->lastCandCount = w[0];
  c->detCnt[DT_LAST_ACCEPTED] = w[0];
  *nrec = w[recWord];
  if (w[0] > cap || *nrec <= spec) return MODSX_OK;
  c->detCnt[DT_SECOND_COPIES]++;
  if (!c->hCand.ensure((size_t)*nrec * sizeof(Candidate))) return MODSX_ERR_NOMEM;   // (re-allocation loses the first part: copy all)
  MX_HIP(ctx_copy(c, c->hCand.p, devRecords, (size_t)*nrec * sizeof(Candidate), hipMemcpyDeviceToHost));
  MX_HIP(ctx_sync(c));
  return MODSX_OK;
}

// the scale-space keypoint of a localised candidate (pyramid.cpp:425-436); the scale through the host's powf
static modsx_sskp sskp_from_candidate(const Candidate &q, const Pyramid &py, const SigmaPlan &sp, int numberOfScales) {
  const float pixelDistance = py.oct[q.octave].pixelDistance;
  const float curScale = sp.curSigma[q.level];
  float scale = curScale * powf(2.0f, q.b2 / numberOfScales);
  modsx_sskp kp;
  kp.octave = q.octave; kp.level = q.level; kp.r0 = q.r0; kp.c0 = q.c0; kp.r = q.r; kp.c = q.c; kp.type = q.type;
  kp.pad = 0;
  kp.b0 = q.b0; kp.b1 = q.b1; kp.b2 = q.b2; kp.val = q.val;
  kp.x = pixelDistance * (q.c + q.b0);
  kp.y = pixelDistance * (q.r + q.b1);
  kp.s = pixelDistance * scale;
  kp.pixelDistance = pixelDistance;
  return kp;
}

// imgStart[i] .. imgStart[i + 1]: where image i's records go when the nrec records are grouped by image
static std::vector<uint32_t> image_starts(const Candidate *cd, unsigned nrec, int n) {
  std::vector<uint32_t> imgStart(n + 1, 0);
  for (unsigned k = 0; k < nrec; k++) imgStart[cd[k].img + 1]++;
  for (int i = 0; i < n; i++) imgStart[i + 1] += imgStart[i];
  return imgStart;
}

// The reference visits (octave, level, row, col) in this order per image (pyramid.cpp:438-451, 490-498, 564-571) and the
// first candidate in that order that lands on a pixel of an octave claims it (octaveMap, :414-418).  Images are
// independent: the candidates are bucketed by image once, then every image sorts one 64-bit key per candidate, applies the
// claim through a small open-addressing table and builds its keypoints -- one task per image on the host pool.
static int order_on_host(modsx_ctx *c, int n, const modsx_hessaff_params &p, std::vector<modsx_sskp> *out) {
  unsigned cnt = 0;
  int rc = download_counted(c, c->cand.p, 0, CAND_CAP, c->lastCandCount, &cnt);
  if (rc) return rc;
  HostMark hm;
  const Candidate *cd = (const Candidate *)c->hCand.p;
  for (unsigned k = 0; k < cnt; k++) {
    const Candidate &q = cd[k];
    if ((unsigned)q.img >= (unsigned)n || (unsigned)q.octave >= 32u || (unsigned)q.level >= 32u || (unsigned)q.r0 >= (1u << 14) ||
        (unsigned)q.c0 >= (1u << 14) || (unsigned)q.r >= (1u << 24) || (unsigned)q.c >= (1u << 24)) {
      set_error("candidate outside the sort key's range");
      return MODSX_ERR_DEVICE;
    }
  }
  std::vector<uint32_t> &byImg = c->candOrder;
  const std::vector<uint32_t> imgStart = image_starts(cd, cnt, n);
  byImg.resize(cnt);
  {
    std::vector<uint32_t> fill(imgStart.begin(), imgStart.end() - 1);
    for (unsigned k = 0; k < cnt; k++) byImg[fill[cd[k].img]++] = k;
  }
  hm.mark("cand bucket by image");
  const SigmaPlan sp = make_sigma_plan(p);
  host_parallel_light(n, [&](int img) {
    std::vector<modsx_sskp> &dst = out[img];
    dst.clear();
    const uint32_t *idx = byImg.data() + imgStart[img];
    const size_t m = imgStart[img + 1] - imgStart[img];
    if (!m) return;
    // keys are unique (one candidate per (octave, level, pixel)), so the order is the same whatever sorts them.  Key and index
    // share ONE 64-bit word (octave 5 | level 5 | row 14 | column 14 | index 21 bits: images are at most 16384 px per side, a set
    // holds at most 2^21 candidates): half the bytes per pass of (key, index) pairs
    static thread_local std::vector<uint64_t> order, order2;
    static_assert(CAND_CAP <= (1u << 21), "index field of the packed sort key");
    order.resize(m);
    for (size_t k = 0; k < m; k++) {
      const Candidate &q = cd[idx[k]];
      order[k] = ((uint64_t)q.octave << 54) | ((uint64_t)q.level << 49) | ((uint64_t)(q.r0 & 0x3fff) << 35) | ((uint64_t)(q.c0 & 0x3fff) << 21) | idx[k];
    }
    host_radix_sort_u64(order, order2, 21, 58);
    size_t tabSize = 64;
    while (tabSize < m * 2 + 16) tabSize <<= 1;
    std::vector<uint64_t> claimed(tabSize, 0);  // key + 1, 0 = empty
    dst.reserve(m);
    for (size_t kk = 0; kk < m; kk++) {
      const Candidate &q = cd[order[kk] & 0x1fffffu];
      const uint64_t key = (((uint64_t)q.octave << 48) | ((uint64_t)q.r << 24) | (uint64_t)q.c) + 1;
      size_t h = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & (tabSize - 1);
      bool taken = false;
      while (claimed[h]) { if (claimed[h] == key) { taken = true; break; } h = (h + 1) & (tabSize - 1); }
      if (taken) continue;
      claimed[h] = key;
      dst.push_back(sskp_from_candidate(q, c->pyr[q.img], sp, p.numberOfScales));
    }
  });
  hm.mark("octaveMap claim + sskp");
  return MODSX_OK;
}

// the opt-in device order lives in libmodsx_cand.so beside this library (kernels_cand.hip), loaded on first use; both entries
// are null when the library or a symbol is missing
struct CandLibrary {
  size_t (*sort_temp_bytes)(unsigned) = nullptr;
  int (*order)(hipStream_t, const Candidate *, const unsigned *, unsigned, unsigned long long *, unsigned long long *, unsigned *, unsigned *,
               void *, size_t, unsigned long long *, unsigned *, unsigned, unsigned *, Candidate *, unsigned *) = nullptr;
};
static const CandLibrary &load_cand_library() {
  static CandLibrary lib;
  static std::once_flag candOnce;
  std::call_once(candOnce, [] {
    Dl_info di;
    std::string path = "libmodsx_cand.so";
    if (dladdr((const void *)&modsx_create, &di) && di.dli_fname) {
      const std::string self(di.dli_fname);
      const size_t sl = self.rfind('/');
      if (sl != std::string::npos) path = self.substr(0, sl + 1) + "libmodsx_cand.so";
    }
    if (void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL)) {
      lib.sort_temp_bytes = (decltype(lib.sort_temp_bytes))dlsym(h, "modsx_cand_sort_temp_bytes");
      lib.order = (decltype(lib.order))dlsym(h, "modsx_cand_order");
    }
  });
  return lib;
}

// MODSX_DEVICE_ORDER=1: detection order and the octaveMap claim on the device (kernels_cand.hip) -- the host receives the
// SURVIVING candidates in the reference's visiting order and only forms the scale (glibc powf) and the keypoint records.
// Built and bit-exact (tests/test_gpu_parity.py), but NOT the default: measured in round 4 it costs the 31-view bench 9 %
// (167 against 183.5 pairs/s) and a lone pair 0.5 ms (13.05 against 12.55 ms) -- key build, radix sort, two table fills, claim
// and compaction are six more small launches on every launch set's stream, while the host's radix sort + hash claim run on
// host cores that are otherwise idle and overlap the other contexts' device work.
static int order_on_device(modsx_ctx *c, int n, const modsx_hessaff_params &p, std::vector<modsx_sskp> *out) {
  const CandLibrary &lib = load_cand_library();
  if (!lib.sort_temp_bytes || !lib.order) {
    set_error("MODSX_DEVICE_ORDER=1, but libmodsx_cand.so (make -C mods_amd/csrc cand) is not beside libmodsx.so");
    return MODSX_ERR_DEVICE;
  }
  unsigned nsurv = 0;
  for (int attempt = 0;; attempt++) {
    // the sort runs over a host-chosen capacity (the device-side count is not known here): what the context's last set had
    // (+ 1/4); a set that holds more is ordered again with its real count -- one more wait, as for the old download
    const unsigned nsort = (unsigned)std::min<size_t>(CAND_CAP, attempt ? c->lastCandCount + 64 : c->lastCandCount + c->lastCandCount / 4 + 1024);
    unsigned tabSize = 1024;
    while (tabSize < 2 * nsort + 16) tabSize <<= 1;
    const size_t tempB = lib.sort_temp_bytes(nsort);
    const size_t keyB = align_up((size_t)nsort * 8, 256), idxB = align_up((size_t)nsort * 4, 256);
    const size_t oKeys = 0, oKeys2 = oKeys + keyB, oIdx = oKeys2 + keyB, oIdx2 = oIdx + idxB, oSlot = oIdx2 + idxB, oTabK = oSlot + idxB,
                 oTabR = oTabK + align_up((size_t)tabSize * 8, 256), oTemp = oTabR + align_up((size_t)tabSize * 4, 256),
                 total = oTemp + align_up(tempB, 256) + 256;
    if (!c->candSort.ensure(total) || !c->candOut.ensure((size_t)nsort * sizeof(Candidate) + 64)) return MODSX_ERR_NOMEM;
    char *w = (char *)c->candSort.p;
    unsigned *survivors = (unsigned *)c->counter.p + 2;     // word 2 of the counter block (zeroed with it)
    if (lib.order(c->stream, (const Candidate *)c->cand.p, (const unsigned *)c->counter.p, nsort, (unsigned long long *)(w + oKeys),
                  (unsigned long long *)(w + oKeys2), (unsigned *)(w + oIdx), (unsigned *)(w + oIdx2), w + oTemp, tempB,
                  (unsigned long long *)(w + oTabK), (unsigned *)(w + oTabR), tabSize, (unsigned *)(w + oSlot),
                  (Candidate *)c->candOut.p, survivors)) { set_error("device-side detection order failed"); return MODSX_ERR_DEVICE; }
    int rc = download_counted(c, c->candOut.p, 2, nsort, c->lastSurvivors, &nsurv);
    if (rc) return rc;
    if (c->lastCandCount <= nsort) break;
    // the capacity was a guess and too small: once more with the count
    if (attempt) { set_error("device-side detection order: capacity does not converge"); return MODSX_ERR_INTERNAL; }
  }
  c->lastSurvivors = nsurv;
  HostMark hm;
  const Candidate *cd = (const Candidate *)c->hCand.p;
  const SigmaPlan sp = make_sigma_plan(p);
  // image-major, then (octave, level, row, column): one linear pass
  for (unsigned k = 0; k < nsurv; k++)
    if ((unsigned)cd[k].img >= (unsigned)n || (unsigned)cd[k].octave >= 32u) { set_error("candidate outside the image / octave range"); return MODSX_ERR_DEVICE; }
  const std::vector<uint32_t> imgStart = image_starts(cd, nsurv, n);
  host_parallel_light(n, [&](int img) {
    std::vector<modsx_sskp> &dst = out[img];
    dst.clear();
    dst.reserve(imgStart[img + 1] - imgStart[img]);
    for (uint32_t k = imgStart[img]; k < imgStart[img + 1]; k++) dst.push_back(sskp_from_candidate(cd[k], c->pyr[cd[k].img], sp, p.numberOfScales));
  });
  hm.mark("sskp from ordered survivors");
  return MODSX_OK;
}

int detect_scalespace_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_hessaff_params &p,
                            std::vector<modsx_sskp> *out) {
  int rc = build_pyramids(c, imgs, n, p, false);
  if (!rc) rc = scan_extrema(c, n, p);
  if (rc) return rc;
  static const bool deviceOrder = getenv("MODSX_DEVICE_ORDER") != nullptr && atoi(getenv("MODSX_DEVICE_ORDER")) != 0;
  return deviceOrder ? order_on_device(c, n, p, out) : order_on_host(c, n, p, out);
}

// Test entry (modsx_debug_pyramids): build_pyramids on a batch, every plane handed back.  geo[49 i ..] = image i's octave count,
// then rows, cols of its octaves; planes (may be null: geometry only, nothing is launched) receives image after image, octave
// after octave, the L blur planes and then the L response planes of the octave -- the layout of Pyramid::store.
int debug_pyramids(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_hessaff_params &p, int *geo, float *planes,
                   unsigned long long capFloats, unsigned long long *needFloats) {
  if (n <= 0 || n > MAXB) { set_error("batch size"); return MODSX_ERR_ARG; }
  if (p.numberOfScales < 1 || p.numberOfScales > 6) { set_error("numberOfScales"); return MODSX_ERR_ARG; }
  if (p.border < 1) { set_error("border must be at least 1"); return MODSX_ERR_ARG; }
  const int L = p.numberOfScales + 2;
  int rc = MODSX_OK, maxOct = 0;
  if (planes) rc = build_pyramids(c, imgs, n, p, false);
  else rc = plan_octaves(c, imgs, n, L, 2 * p.border + 2, false, &maxOct);
  if (rc) return rc;
  unsigned long long total = 0;
  for (int i = 0; i < n; i++) {
    const Pyramid &py = c->pyr[i];
    int *g = geo + 49 * i;
    g[0] = py.nOct;
    unsigned long long mine = 0;
    for (int o = 0; o < py.nOct; o++) { g[1 + 2 * o] = py.oct[o].rows; g[2 + 2 * o] = py.oct[o].cols; mine += (unsigned long long)2 * L * py.oct[o].rows * py.oct[o].cols; }
    if (planes && mine) {
      if (total + mine > capFloats) { set_error("modsx_debug_pyramids: the plane buffer is too small"); return MODSX_ERR_ARG; }
      MX_HIP(hipMemcpyAsync(planes + total, py.store.p, mine * 4, hipMemcpyDeviceToHost, c->stream));
    }
    total += mine;
  }
  *needFloats = total;
  if (planes) MX_HIP(hipStreamSynchronize(c->stream));
  return MODSX_OK;
}

// Test entry (modsx_debug_scan_levels): the production scan_extrema + order_on_host on the L = numberOfScales + 2 response and
// blur planes of ONE octave that the caller supplies (they become octave 0 of the context's first pyramid).  cands: the accepted
// records as the device appended them (any order); out: the keypoints after the detection order and the octaveMap claim.
int debug_scan_levels(modsx_ctx *c, const float *resps, const float *blurs, int L, int rows, int cols, const modsx_hessaff_params &p,
                      std::vector<Candidate> &cands, std::vector<modsx_sskp> &out) {
  if (p.numberOfScales < 1 || p.numberOfScales > 6 || L != p.numberOfScales + 2) { set_error("modsx_debug_scan_levels: numberOfScales + 2 planes are expected"); return MODSX_ERR_ARG; }
  if (p.border < 1) { set_error("border must be at least 1"); return MODSX_ERR_ARG; }
  if (p.detectorType != MODSX_DET_HESSIAN && p.detectorType != MODSX_DET_DOG && p.detectorType != MODSX_DET_HARRIS) {
    set_error("detectorType must be Hessian (0), DoG (1) or Harris (2)");
    return MODSX_ERR_ARG;
  }
  if (rows < 1 || cols < 1 || rows >= (1 << 14) || cols >= (1 << 14)) { set_error("modsx_debug_scan_levels: plane size"); return MODSX_ERR_ARG; }
  Pyramid &py = c->pyr[0];
  const size_t npx = (size_t)rows * cols;
  if (!py.store.ensure((size_t)2 * L * npx * sizeof(float) + 64)) return MODSX_ERR_NOMEM;
  py.nOct = 1;
  Octave &oc = py.oct[0];
  oc.rows = rows; oc.cols = cols; oc.pixelDistance = 1.0f;
  float *ptr = (float *)py.store.p;
  for (int l = 0; l < L; l++) { oc.blur[l] = ptr; ptr += npx; }
  for (int l = 0; l < L; l++) { oc.resp[l] = ptr; ptr += npx; }
  MX_HIP(hipMemcpyAsync(oc.blur[0], blurs, (size_t)L * npx * 4, hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipMemcpyAsync(oc.resp[0], resps, (size_t)L * npx * 4, hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));    // the caller's planes are its own again
  int rc = scan_extrema(c, 1, p);
  std::vector<modsx_sskp> kp[1];
  if (!rc) rc = order_on_host(c, 1, p, kp);
  if (rc) return rc;
  const Candidate *cd = (const Candidate *)c->hCand.p;
  cands.assign(cd, cd + c->lastCandCount);
  out.swap(kp[0]);
  return MODSX_OK;
}

static int ensure_smm_mask(modsx_ctx *c, int W) {
  if (c->smmW == W && c->dSmmMask) return MODSX_OK;
  if (W < 3 || W > 19 || !(W & 1)) { set_error("smmWindowSize must be odd and <= 19"); return MODSX_ERR_ARG; }
  if (c->dSmmMask) hipFree(c->dSmmMask);
  std::vector<float> m(W * W);
  gauss_mask(m.data(), W);
  MX_HIP(hipMalloc(&c->dSmmMask, W * W * 4));
  MX_HIP(hipMemcpy(c->dSmmMask, m.data(), W * W * 4, hipMemcpyHostToDevice));
  c->smmW = W;
  return MODSX_OK;
}

// baumberg_geometry as this context launches: the production rule of the queue form counts the resident wavefronts of its device
int debug_baumberg_geometry(modsx_ctx *c, int n, int W, int variant, int chunk, int *geo) {
  const BaumGeo g = baumberg_geometry(n, W, variant, chunk, baum_resident(c));
  geo[0] = g.kernel; geo[1] = g.chunk; geo[2] = g.nchunks; geo[3] = g.grid;
  if (g.kernel < 0) { set_error("modsx_debug_baumberg_geometry_ctx: no kernel for this window size / variant / chunk"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

// Test entry (modsx_debug_baumberg): a Baumberg launch on a caller's job list, through the production launcher.  Job k reads
// planes[planeOf[k]] at xyspd[4k ..] = x, y, s, pixelDistance.  The result buffer is filled with 0xFF bytes first, so a keypoint
// that no wavefront wrote shows iters == -1.  geo: what baumberg_geometry gives for the launch.  handedOut (may be null): the
// keypoints the counters of the queue form handed out, each counter clipped to the length of its range (0 for the other kernels).
int debug_baumberg(modsx_ctx *c, const modsx_image *const *planes, int nplanes, const int *planeOf, const float *xyspd, int n,
                   const modsx_hessaff_params &p, int variant, int chunk, float *u, int *ok, int *iters, int *geo, int *handedOut) {
  const BaumGeo g = baumberg_geometry(n, p.smmWindowSize, variant, chunk, baum_resident(c));
  if (handedOut) *handedOut = 0;
  if (g.kernel < 0) { set_error("modsx_debug_baumberg: no kernel for this window size / variant / chunk"); return MODSX_ERR_ARG; }
  geo[0] = g.kernel; geo[1] = g.chunk; geo[2] = g.nchunks; geo[3] = g.grid;
  for (int i = 0; i < nplanes; i++)
    if (!planes[i] || !planes[i]->d || planes[i]->rows < 4 || planes[i]->cols < 4) { set_error("modsx_debug_baumberg: planes must be at least 4 x 4"); return MODSX_ERR_ARG; }
  for (int k = 0; k < n; k++) {
    const float *q = xyspd + 4 * (size_t)k;
    if ((unsigned)planeOf[k] >= (unsigned)nplanes || !std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]) ||
        !(q[3] > 0.f) || !std::isfinite(q[3])) {
      set_error("modsx_debug_baumberg: job outside the contract (plane index, finite x / y / s, pixelDistance > 0)");
      return MODSX_ERR_ARG;
    }
  }
  if (!n) return MODSX_OK;
  int rc = ensure_smm_mask(c, p.smmWindowSize);
  if (rc) return rc;
  const size_t total = (size_t)n;
  if (!c->hAff.ensure(total * sizeof(AffJob) + total * sizeof(AffOut))) return MODSX_ERR_NOMEM;
  if (!c->affJobs.ensure(total * sizeof(AffJob)) || !c->affOut.ensure(total * sizeof(AffOut))) return MODSX_ERR_NOMEM;
  if (!c->counter.ensure(COUNTER_BYTES) || !c->hMisc.ensure(BAUM_QUEUE_BYTES)) return MODSX_ERR_NOMEM;
  AffJob *hj = (AffJob *)c->hAff.p;
  AffOut *ho = (AffOut *)((char *)c->hAff.p + total * sizeof(AffJob));
  for (int k = 0; k < n; k++) {
    const modsx_image *im = planes[planeOf[k]];
    const float *q = xyspd + 4 * (size_t)k;
    AffJob &j = hj[k];
    j.blur = im->d; j.rows = im->rows; j.cols = im->cols;
    j.x = q[0]; j.y = q[1]; j.s = q[2]; j.pixelDistance = q[3];
  }
  hipStream_t s = c->stream;
  MX_HIP(hipMemcpyAsync(c->affJobs.p, hj, total * sizeof(AffJob), hipMemcpyHostToDevice, s));
  MX_HIP(hipMemsetAsync(c->affOut.p, 0xFF, total * sizeof(AffOut), s));
  // (no scan has filled the counter block for this launch: the launcher zeroes the queue's counters)
  if (!launch_baumberg(s, (AffJob *)c->affJobs.p, (AffOut *)c->affOut.p, n, c->dSmmMask, p.smmWindowSize, p.maxIterations,
                       p.convergenceThreshold, p.affInitialSigma, variant, chunk, baum_resident(c), baum_queue(c), false)) {
    MX_HIP(hipGetLastError());
    set_error("modsx_debug_baumberg: nothing was launched"); return MODSX_ERR_INTERNAL;
  }
  MX_HIP(hipGetLastError());
  MX_HIP(hipMemcpyAsync(ho, c->affOut.p, total * sizeof(AffOut), hipMemcpyDeviceToHost, s));
  if (g.kernel == 3) MX_HIP(hipMemcpyAsync(c->hMisc.p, baum_queue(c), BAUM_QUEUE_BYTES, hipMemcpyDeviceToHost, s));
  MX_HIP(hipStreamSynchronize(s));
  if (g.kernel == 3 && handedOut) {
    const unsigned *w = (const unsigned *)c->hMisc.p;
    for (int r = 0; r < BAUM_RANGES; r++) {
      const unsigned len = (unsigned)(baum_range_start(n, r + 1) - baum_range_start(n, r));
      *handedOut += (int)std::min(w[BAUM_COUNTER_STRIDE * r], len);
    }
  }
  for (int k = 0; k < n; k++) {
    u[4 * k] = ho[k].u11; u[4 * k + 1] = ho[k].u12; u[4 * k + 2] = ho[k].u21; u[4 * k + 3] = ho[k].u22;
    ok[k] = ho[k].ok; iters[k] = ho[k].iters;
  }
  return MODSX_OK;
}

// ------------------------------------------------------------------------------------------------
// External affine adaptation: DetectAffineShape (synth-detection.cpp:922-1074) on a caller's regions
// ------------------------------------------------------------------------------------------------
int affshape_check(const char *fn, const modsx_affshape_params &p) {
  if (p.smmWindowSize < 3 || p.smmWindowSize > 19 || !(p.smmWindowSize & 1)) {
    set_error(std::string(fn) + ": smmWindowSize must be odd and in 3..19"); return MODSX_ERR_ARG;
  }
  if (p.affBmbrgMethod != 0) {
    set_error(std::string(fn) + ": affBmbrgMethod must be 0 (AFF_BMBRG_SMM); AFF_BMBRG_HESSIAN needs cv::SVD and is not built");
    return MODSX_ERR_ARG;
  }
  if (!std::isfinite(p.convergenceThreshold)) { set_error(std::string(fn) + ": convergenceThreshold must be finite"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

// The host's share of a region (synth-detection.cpp:949-964).  ratio: `float ratio = det_kp.s / initialSigma` with s a double and
// initialSigma the function's `const float 1.6` -- an f64 division rounded once; the window argument `2*5.0*ratio` is the double
// 10.0 * ratio, which the int parameter of interpolateCheckBorders truncates.
int affshape_jobs(const char *fn, const modsx_region *in, int n, int cols, int rows, float *ratio, int *res, unsigned char *border) {
  if (n < 0 || (n > 0 && !in)) { set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
  if (rows < 4 || cols < 4) { set_error(std::string(fn) + ": images must be at least 4 x 4"); return MODSX_ERR_ARG; }
  const float initialSigma = 1.6f;
  for (int k = 0; k < n; k++) {
    const modsx_keypoint &q = in[k].det_kp;
    if (!std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.s) || !std::isfinite(q.a11) || !std::isfinite(q.a12) ||
        !std::isfinite(q.a21) || !std::isfinite(q.a22)) {
      set_error(std::string(fn) + ": region " + std::to_string(k) + " has a non-finite x, y, s or matrix entry"); return MODSX_ERR_ARG;
    }
    const float r = (float)(q.s / (double)initialSigma);
    const double w = 2 * 5.0 * r;
    if (!(fabs(w) < 2147483648.0)) {
      set_error(std::string(fn) + ": region " + std::to_string(k) + ": |10 * s / 1.6| must be below 2^31"); return MODSX_ERR_ARG;
    }
    const int rs = (int)w;
    if (ratio) ratio[k] = r;
    if (res) res[k] = rs;
    if (border) border[k] = check_borders_host(cols, rows, (float)q.x, (float)q.y, (float)q.a11, (float)q.a12, (float)q.a21, (float)q.a22, rs, rs) ? 1 : 0;
  }
  return n;
}

int affine_shape_batch(modsx_ctx *c, const char *fn, const modsx_image *const *imgs, int nImgs, const modsx_region *in, const int *counts,
                       const modsx_affshape_params &p, int variant, std::vector<modsx_region> *out, const AffShapeReport *rep) {
  int rc = affshape_check(fn, p);
  if (rc) return rc;
  const int W = p.smmWindowSize;
  if (variant < 0) variant = baumberg_production_variant(W);
  size_t total = 0;
  for (int i = 0; i < nImgs; i++) {
    if (!imgs[i] || !imgs[i]->d || counts[i] < 0) { set_error(std::string(fn) + ": bad argument"); return MODSX_ERR_ARG; }
    total += (size_t)counts[i];
  }
  if (total > (size_t)1 << 28) { set_error(std::string(fn) + ": too many regions"); return MODSX_ERR_ARG; }
  std::vector<float> ratio(total);
  std::vector<unsigned char> border(total);
  {
    size_t k = 0;
    for (int i = 0; i < nImgs; k += (size_t)counts[i], i++) {
      rc = affshape_jobs(fn, in + k, counts[i], imgs[i]->cols, imgs[i]->rows, ratio.data() + k, nullptr, border.data() + k);
      if (rc < 0) return rc;
    }
  }
  size_t launched = 0;
  for (size_t k = 0; k < total; k++) launched += !border[k];
  const BaumGeo g = baumberg_geometry((int)launched, W, variant, 0, baum_resident(c));
  if (g.kernel < 0) {
    if (variant == 3 && W == 19 && !baum_resident(c)) {
      set_error(std::string(fn) + ": the occupancy query that sizes the queue form's grid failed (MODSX_BAUMBERG_QUEUE=0 runs the static chunks)");
      return MODSX_ERR_DEVICE;
    }
    set_error(std::string(fn) + ": no kernel for this window size / variant"); return MODSX_ERR_ARG;
  }
  if (rep && rep->geo) { rep->geo[0] = g.kernel; rep->geo[1] = g.chunk; rep->geo[2] = g.nchunks; rep->geo[3] = g.grid; }
  if (out) for (int i = 0; i < nImgs; i++) out[i].clear();
  if (rep)
    for (size_t k = 0; k < total; k++) {
      if (rep->border) rep->border[k] = border[k];
      if (rep->u) { rep->u[4 * k] = 1.f; rep->u[4 * k + 1] = 0.f; rep->u[4 * k + 2] = 0.f; rep->u[4 * k + 3] = 1.f; }
      if (rep->ok) rep->ok[k] = 0;
      if (rep->iters) rep->iters[k] = border[k] ? -1 : 0;
    }
  c->affshapeCounters[0]++;
  c->affshapeCounters[1] += (long)total;
  c->affshapeCounters[2] += (long)(total - launched);
  if (!launched || p.maxIterations <= 0) return (int)launched;   // the reference's loop does not run: nothing converges
  rc = ensure_smm_mask(c, W);
  if (rc) return rc;
  CtxBusy busy(c);
  if (!c->hAff.ensure(launched * sizeof(AffJob) + launched * sizeof(AffOut))) return MODSX_ERR_NOMEM;
  if (!c->affJobs.ensure(launched * sizeof(AffJob)) || !c->affOut.ensure(launched * sizeof(AffOut))) return MODSX_ERR_NOMEM;
  if (!c->counter.ensure(COUNTER_BYTES)) return MODSX_ERR_NOMEM;
  AffJob *hj = (AffJob *)c->hAff.p;
  AffOut *ho = (AffOut *)((char *)c->hAff.p + launched * sizeof(AffJob));
  {
    size_t k = 0, j = 0;
    for (int i = 0; i < nImgs; i++)
      for (int r = 0; r < counts[i]; r++, k++) {
        if (border[k]) continue;
        AffJob &a = hj[j++];
        a.blur = imgs[i]->d; a.rows = imgs[i]->rows; a.cols = imgs[i]->cols;
        a.x = (float)in[k].det_kp.x; a.y = (float)in[k].det_kp.y; a.s = ratio[k]; a.pixelDistance = 1.f;
      }
  }
  hipStream_t s = c->stream;
  MX_HIP(ctx_copy(c, c->affJobs.p, hj, launched * sizeof(AffJob), hipMemcpyHostToDevice));
  if (rep) MX_HIP(hipMemsetAsync(c->affOut.p, 0xFF, launched * sizeof(AffOut), s));   // the test entry: a job no wavefront wrote shows iters == -1
  {
    ProfScope ps(c, K_BAUMBERG, (double)launched * W * W * 4 * 2);
    // no scan has filled the counter block for this launch: the launcher zeroes the queue's counters itself.  A later detection
    // call starts with scan_extrema's fill of the whole block, so what this launch leaves in them is never read
    if (!launch_baumberg_external(s, (AffJob *)c->affJobs.p, (AffOut *)c->affOut.p, (int)launched, c->dSmmMask, W, p.maxIterations,
                                  p.convergenceThreshold, variant, 0, baum_resident(c), baum_queue(c), false)) {
      MX_HIP(hipGetLastError());
      set_error(std::string(fn) + ": nothing was launched"); return MODSX_ERR_INTERNAL;
    }
  }
  MX_HIP(hipGetLastError());
  MX_HIP(ctx_copy(c, ho, c->affOut.p, launched * sizeof(AffOut), hipMemcpyDeviceToHost));
  MX_HIP(ctx_sync(c));
  c->affshapeCounters[3] += (long)launched;
  c->affshapeCounters[5]++;
  {
    size_t k = 0, j = 0;
    for (int i = 0; i < nImgs; i++)
      for (int r = 0; r < counts[i]; r++, k++) {
        if (border[k]) continue;
        const AffOut &a = ho[j++];
        if (rep) {
          if (rep->u) { rep->u[4 * k] = a.u11; rep->u[4 * k + 1] = a.u12; rep->u[4 * k + 2] = a.u21; rep->u[4 * k + 3] = a.u22; }
          if (rep->ok) rep->ok[k] = a.ok;
          if (rep->iters) rep->iters[k] = a.iters;
        }
        if (!a.ok) continue;
        c->affshapeCounters[4]++;
        if (!out) continue;
        out[i].push_back(in[k]);
        modsx_keypoint &q = out[i].back().det_kp;
        q.a11 = (double)a.u11; q.a12 = (double)a.u12; q.a21 = (double)a.u21; q.a22 = (double)a.u22;
      }
  }
  return (int)launched;
}

// AffineDetector::prepareKeysForExport, scale-space-detector.hpp:118-198
static void prepare_keys_for_export(std::vector<modsx_keypoint> &keys, const modsx_hessaff_params &p) {
  if (keys.empty() || p.mode == MODSX_FIXED_TH) return;
  auto cmpv = [](modsx_keypoint k1, modsx_keypoint k2) { return fabs(k1.response) > fabs(k2.response); };
  std::sort(keys.begin(), keys.end(), cmpv);
  double maxResponse = fabs(keys[0].response);
  int regNumber = (int)keys.size();
  auto cmp = [](const modsx_keypoint &k1, const modsx_keypoint &k2) { return fabs(k1.response) > fabs(k2.response); };
  switch (p.mode) {
    case MODSX_RELATIVE_TH: {
      modsx_keypoint t = keys[0];
      t.response = (float)(maxResponse * p.rel_threshold);
      keys.resize(std::lower_bound(keys.begin(), keys.end(), t, cmp) - keys.begin());
      break;
    }
    case MODSX_FIXED_REG_NUMBER: {
      int nn = p.reg_number;
      if (p.doBaumberg) nn = (int)floor(3.0 * (double)nn);
      if ((nn < regNumber) && (nn >= 0)) keys.resize(nn);
      break;
    }
    case MODSX_RELATIVE_REG_NUMBER: {
      keys.resize((int)floor(p.rel_reg_number * (double)keys.size()));
      break;
    }
    case MODSX_NOT_LESS_THAN_REGIONS: {
      modsx_keypoint t = keys[0];
      t.response = p.threshold;
      int fix = (int)(std::lower_bound(keys.begin(), keys.end(), t, cmp) - keys.begin());
      if (fix < p.reg_number) keys.resize(std::min(p.reg_number, regNumber));
      else keys.resize(std::min(fix, regNumber));
      break;
    }
    default: break;
  }
  if (p.mode == MODSX_FIXED_REG_NUMBER && (int)keys.size() > p.reg_number) keys.resize(p.reg_number);
}

// DetectAffineKeypoints (scale-space-detector.cpp:43-85) for a batch of images
int detect_keypoints_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_hessaff_params &par,
                           const double *tilts, const double *zooms, std::vector<modsx_keypoint> *out) {
  modsx_hessaff_params p = par;  // reg_number is rescaled per image just before the export step (it only matters there)
  std::vector<modsx_sskp> ss[MAXB];
  int rc = detect_scalespace_batch(c, imgs, n, p, ss);
  if (rc) return rc;
  HostMark hm;
  rc = ensure_smm_mask(c, p.smmWindowSize);
  if (rc) return rc;
  size_t total = 0;
  for (int i = 0; i < n; i++) total += ss[i].size();
  for (int i = 0; i < n; i++) out[i].clear();
  if (!total) return MODSX_OK;
  hipStream_t s = c->stream;
  if (!c->hAff.ensure(total * sizeof(AffJob) + total * sizeof(AffOut))) return MODSX_ERR_NOMEM;
  if (!c->affJobs.ensure(total * sizeof(AffJob)) || !c->affOut.ensure(total * sizeof(AffOut))) return MODSX_ERR_NOMEM;
  AffJob *hj = (AffJob *)c->hAff.p;
  AffOut *ho = (AffOut *)((char *)c->hAff.p + total * sizeof(AffJob));
  size_t first[MAXB + 1];   // image i's keypoints are jobs first[i] .. first[i + 1]
  first[0] = 0;
  for (int i = 0; i < n; i++) first[i + 1] = first[i] + ss[i].size();
  host_parallel_light(n, [&](int i) {
    size_t k = first[i];
    for (const modsx_sskp &q : ss[i]) {
      const Octave &oc = c->pyr[i].oct[q.octave];
      AffJob &j = hj[k++];
      j.blur = oc.blur[q.level - 1];  // prevBlur: one level below the detection level (pyramid.cpp:428-429)
      j.rows = oc.rows; j.cols = oc.cols;
      j.x = q.x; j.y = q.y; j.s = q.s; j.pixelDistance = q.pixelDistance;
    }
  });
  hm.mark("AffJob build");
  if (p.doBaumberg) {
    MX_HIP(ctx_copy(c, c->affJobs.p, hj, total * sizeof(AffJob), hipMemcpyHostToDevice));
    ProfScope ps(c, K_BAUMBERG, (double)total * 361 * 4 * 2);
    // (the queue's counters are zero since scan_extrema's fill of the counter block)
    const int variant = baumberg_production_variant(p.smmWindowSize);
    if (variant == 3 && !baum_resident(c)) {
      set_error("Baumberg: the occupancy query that sizes the queue form's grid failed (MODSX_BAUMBERG_QUEUE=0 runs the static chunks)");
      return MODSX_ERR_DEVICE;
    }
    if (!launch_baumberg(s, (AffJob *)c->affJobs.p, (AffOut *)c->affOut.p, (int)total, c->dSmmMask, p.smmWindowSize, p.maxIterations,
                         p.convergenceThreshold, p.affInitialSigma, variant, 0, baum_resident(c), baum_queue(c), true)) {
      MX_HIP(hipGetLastError());
      set_error("Baumberg: no kernel for this window size"); return MODSX_ERR_INTERNAL;
    }
    MX_HIP(ctx_copy(c, ho, c->affOut.p, total * sizeof(AffOut), hipMemcpyDeviceToHost));
    MX_HIP(ctx_sync(c));
  } else {
    for (size_t i = 0; i < total; i++) { ho[i].u11 = 1; ho[i].u12 = 0; ho[i].u21 = 0; ho[i].u22 = 1; ho[i].ok = 1; ho[i].iters = 0; }
  }
  hm.mark("baumberg launch + wait");
  host_parallel_light(n, [&](int i) {
    size_t k = first[i];
    out[i].reserve(ss[i].size());
    for (const modsx_sskp &q : ss[i]) {
      const AffOut &a = ho[k++];
      if (!a.ok) continue;
      modsx_keypoint kp;
      memset(&kp, 0, sizeof kp);
      kp.x = q.x; kp.y = q.y; kp.s = q.s;
      kp.a11 = a.u11; kp.a12 = a.u12; kp.a21 = a.u21; kp.a22 = a.u22;
      kp.response = q.val;
      kp.sub_type = q.type;
      out[i].push_back(kp);
    }
    modsx_hessaff_params pe = p;
    const double tilt = tilts ? tilts[i] : 1.0, zoom = zooms ? zooms[i] : 1.0;
    if ((tilt > 2.0) || (zoom < 0.5)) pe.reg_number = (int)floor(zoom * (double)pe.reg_number / tilt);
    prepare_keys_for_export(out[i], pe);
  });
  hm.mark("keypoints + export");
  return MODSX_OK;
}

// DetectAffineRegions<>, synth-detection.hpp:93-126
void detect_affine_regions(const modsx_keypoint *kps, int n, int img_id, int det_type, modsx_region *out) {
  for (int i = 0; i < n; i++) {
    modsx_keypoint k = kps[i];
    modsx_region &r = out[i];         // built in place (a 200-byte record)
    memset(&r, 0, sizeof r);
    r.img_id = img_id; r.img_reproj_id = 0; r.type = det_type; r.id = i;
    r.det_kp.s = k.s * sqrt(fabs(k.a11 * k.a22 - k.a12 * k.a21));
    rectify(k.a11, k.a12, k.a21, k.a22);
    r.det_kp.x = k.x; r.det_kp.y = k.y;
    r.det_kp.a11 = k.a11; r.det_kp.a12 = k.a12; r.det_kp.a21 = k.a21; r.det_kp.a22 = k.a22;
    r.det_kp.response = k.response;
    r.det_kp.sub_type = k.sub_type;
  }
}

}  // namespace mx
