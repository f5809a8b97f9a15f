// engine_surfdet.hip -- the "SURF" detector branch of the reference (imagerepresentation.cpp:1046-1076): Integral of the view, then
// FastHessian(int_img, ipts, octaves, intervals, init_sample, thres).getIpoints(), on the GPU (kernels_surfdet.hip).
//   * surfdet_normalise is saveParameters, surfdet_geometry the layer table of buildResponseMap: host code, shared with the kernels'
//     job table and with modsx_surfdet_geometry;
//   * a call takes its images in launch sets of at most MAXB: one job table, one launch each of the row pass, the column pass, the
//     response layers, the scan and its offsets, then -- once the host has read the counts and made room -- the emit pass;
//   * the number of points is not known up front: the scan counts them, the host reads the per-image totals (the call's first wait)
//     and grows the point buffer when it is too small (counted as a regrow), so a full buffer never drops a point;
//   * keypoints are filled as the branch fills det_kp: x, y, s widened to double, the frame of orientation 0.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>
#include "engine_api.hpp"

namespace mx {

constexpr size_t SD_INIT_POINTS = 256;      // points the buffer holds before its first regrow

modsx_surfdet_params surfdet_normalise(const modsx_surfdet_params &p) {
  modsx_surfdet_params o;
  o.octaves = (p.octaves > 0 && p.octaves <= 4 ? p.octaves : 5);
  o.intervals = (p.intervals > 0 && p.intervals <= 4 ? p.intervals : 4);
  o.init_sample = (p.init_sample > 0 && p.init_sample <= 6 ? p.init_sample : 2);
  o.thresh = (p.thresh >= 0 ? p.thresh : 0.0004f);
  return o;
}

// layers [12][4] = (width, height, step, filter) of buildResponseMap (fasthessian.cpp:131-188); returns their number, or MODSX_ERR_ARG
// where a layer would have width or height 0 (the reference's assert aborts there)
int surfdet_geometry(const char *fn, int rows, int cols, const modsx_surfdet_params &par, int *layers) {
  static const int filters[SD_MAX_LAYERS] = {9, 15, 21, 27, 39, 51, 75, 99, 147, 195, 291, 387};
  if (rows <= 0 || cols <= 0) { set_error(std::string(fn) + ": bad image size"); return MODSX_ERR_ARG; }
  const modsx_surfdet_params p = surfdet_normalise(par);
  const int w = cols / p.init_sample, h = rows / p.init_sample, s = p.init_sample;
  int n = 0;
  for (int o = 0; o < p.octaves; o++) {
    const int d = 1 << o;
    if (w / d <= 0 || h / d <= 0) {
      set_error(std::string(fn) + ": the image is too small for octave " + std::to_string(o + 1) + " at this init_sample (a response layer of width or height 0)");
      return MODSX_ERR_ARG;
    }
    for (int k = (o == 0 ? 0 : 2 + 2 * o); k < 4 + 2 * o; k++, n++)
      if (layers) { layers[4 * n] = w / d; layers[4 * n + 1] = h / d; layers[4 * n + 2] = s * d; layers[4 * n + 3] = filters[k]; }
  }
  return n;
}

int surfdet_check(const char *fn, const modsx_image *const *imgs, int n, const modsx_surfdet_params &par) {
  for (int i = 0; i < n; i++) {
    if (!imgs[i] || !imgs[i]->d) { set_error(std::string(fn) + ": null image"); return MODSX_ERR_ARG; }
    const int rc = surfdet_geometry(fn, imgs[i]->rows, imgs[i]->cols, par, nullptr);
    if (rc < 0) return rc;
  }
  return MODSX_OK;
}

void surf_regions(const modsx_keypoint *kps, int n, int img_id, modsx_region *out) {
  for (int i = 0; i < n; i++) {
    modsx_region &r = out[i];
    memset(&r, 0, sizeof r);
    r.img_id = img_id; r.img_reproj_id = 0; r.type = MODSX_DET_SURF; r.id = i;
    r.det_kp = kps[i];
  }
}

namespace {
struct Plan {       // the tables of one launch set, as they lie in sdHost / sdTab
  std::vector<SdJob> jobs;
  std::vector<SdSeg> rowSegs, colSegs, respSegs, scanSegs;
  std::vector<int> tile0;
  std::vector<size_t> integOfs;      // float offset of every job's integral image in the arena
  int rowBlocks = 0, colBlocks = 0, respBlocks = 0, tiles = 0;
  size_t integFloats = 0, planeValues = 0;
};
}  // namespace

static int make_plan(const modsx_image *const *imgs, int n, const modsx_surfdet_params &p, Plan &pl) {
  static const int filter_map[5][4] = {{0, 1, 2, 3}, {1, 3, 4, 5}, {3, 5, 6, 7}, {5, 7, 8, 9}, {7, 9, 10, 11}};
  for (int j = 0; j < n; j++) {
    SdJob J = {};
    int lay[SD_MAX_LAYERS * 4];
    const int nl = surfdet_geometry("modsx_detect_surf", imgs[j]->rows, imgs[j]->cols, p, lay);
    if (nl < 0) return nl;
    J.src = imgs[j]->d; J.rows = imgs[j]->rows; J.cols = imgs[j]->cols; J.nLayers = nl;
    pl.integOfs.push_back(pl.integFloats);
    pl.integFloats += (size_t)J.rows * J.cols;
    pl.rowSegs.push_back({j, 0, 0, pl.rowBlocks}); pl.rowBlocks += (J.rows + SD_ROWS_PER_WG - 1) / SD_ROWS_PER_WG;
    pl.colSegs.push_back({j, 0, 0, pl.colBlocks}); pl.colBlocks += (J.cols + 63) / 64;
    for (int k = 0; k < nl; k++) {
      SdLayer &L = J.L[k];
      L.w = lay[4 * k]; L.h = lay[4 * k + 1]; L.step = lay[4 * k + 2]; L.filter = lay[4 * k + 3]; L.ofs = pl.planeValues;
      const size_t px = (size_t)L.w * L.h;
      pl.planeValues += px;
      pl.respSegs.push_back({j, k, 0, pl.respBlocks}); pl.respBlocks += (int)((px + SD_TILE - 1) / SD_TILE);
    }
    pl.tile0.push_back(pl.tiles);
    for (int o = 0; o < p.octaves; o++)
      for (int i = 0; i <= 1; i++) {
        const SdLayer &t = J.L[filter_map[o][i + 2]];
        pl.scanSegs.push_back({j, o, i, pl.tiles}); pl.tiles += (int)(((size_t)t.w * t.h + SD_TILE - 1) / SD_TILE);
      }
    pl.jobs.push_back(J);
  }
  pl.tile0.push_back(pl.tiles);
  return MODSX_OK;
}

// what one launch set leaves on the device for the debug tap
struct SurfdetTap {
  float *integral; int *layers; float *resp; unsigned char *lap;
  int *ext; double *dD, *H, *x; int *accepted, *laplacian; int capExt; int *nExt;
};

static int run_set(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_surfdet_params &p, std::vector<modsx_keypoint> *out,
                   const SurfdetTap *tap) {
  Plan pl;
  int rc = make_plan(imgs, n, p, pl);
  if (rc) return rc;
  // one table blob: jobs, the four run tables, tile0, then (device only) jobStart [n + 1][2], offs [tiles + 1][2]
  size_t o = 0;
  auto place = [&](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 16); return at; };
  const size_t oJobs = place(sizeof(SdJob) * n), oRow = place(sizeof(SdSeg) * pl.rowSegs.size()), oCol = place(sizeof(SdSeg) * pl.colSegs.size()),
               oResp = place(sizeof(SdSeg) * pl.respSegs.size()), oScan = place(sizeof(SdSeg) * pl.scanSegs.size()),
               oTile0 = place(sizeof(int) * pl.tile0.size()), hostBytes = o, oStart = place(sizeof(int) * 2 * (n + 1)),
               oOffs = place(sizeof(int) * 2 * ((size_t)pl.tiles + 1));
  if (!c->sdHost.ensure(hostBytes) || !c->sdTab.ensure(o) || !c->sdInteg.ensure(pl.integFloats * 4) || !c->sdResp.ensure(pl.planeValues * 4) ||
      !c->sdLap.ensure(pl.planeValues) || !c->sdFlags.ensure((size_t)pl.tiles * SD_TILE + 1) || !c->sdCounts.ensure((size_t)pl.tiles * 8 + 8) ||
      !c->sdBack.ensure(sizeof(int) * 2 * (n + 1)) || !c->sdPoints.ensure(SD_INIT_POINTS * sizeof(SdPoint)))
    return MODSX_ERR_NOMEM;
  for (int j = 0; j < n; j++) pl.jobs[j].integ = (float *)c->sdInteg.p + pl.integOfs[j];
  char *h = (char *)c->sdHost.p, *d = (char *)c->sdTab.p;
  memcpy(h + oJobs, pl.jobs.data(), sizeof(SdJob) * n);
  memcpy(h + oRow, pl.rowSegs.data(), sizeof(SdSeg) * pl.rowSegs.size());
  memcpy(h + oCol, pl.colSegs.data(), sizeof(SdSeg) * pl.colSegs.size());
  memcpy(h + oResp, pl.respSegs.data(), sizeof(SdSeg) * pl.respSegs.size());
  memcpy(h + oScan, pl.scanSegs.data(), sizeof(SdSeg) * pl.scanSegs.size());
  memcpy(h + oTile0, pl.tile0.data(), sizeof(int) * pl.tile0.size());
  MX_HIP(hipMemcpyAsync(d, h, hostBytes, hipMemcpyHostToDevice, c->stream));
  const SdJob *jobs = (const SdJob *)(d + oJobs);
  const SdSeg *scanSegs = (const SdSeg *)(d + oScan);
  const float *resp = (const float *)c->sdResp.p;
  const unsigned char *lap = (const unsigned char *)c->sdLap.p;
  int *offs = (int *)(d + oOffs);
  launch_surfdet_integral(c->stream, jobs, (const SdSeg *)(d + oRow), (int)pl.rowSegs.size(), pl.rowBlocks, (const SdSeg *)(d + oCol),
                          (int)pl.colSegs.size(), pl.colBlocks);
  launch_surfdet_responses(c->stream, jobs, (const SdSeg *)(d + oResp), (int)pl.respSegs.size(), pl.respBlocks, (float *)c->sdResp.p,
                           (unsigned char *)c->sdLap.p);
  launch_surfdet_scan(c->stream, jobs, scanSegs, (int)pl.scanSegs.size(), pl.tiles, resp, lap, p.thresh, (unsigned char *)c->sdFlags.p,
                      (int *)c->sdCounts.p, offs, (const int *)(d + oTile0), n, (int *)(d + oStart));
  MX_HIP(hipMemcpyAsync(c->sdBack.p, d + oStart, sizeof(int) * 2 * (n + 1), hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  const int *start = (const int *)c->sdBack.p;
  const size_t nExt = (size_t)start[2 * n], nAcc = (size_t)start[2 * n + 1];
  if (nAcc * sizeof(SdPoint) > c->sdPoints.cap) {
    c->sdCounters[4]++;
    if (!c->sdPoints.ensure(nAcc * sizeof(SdPoint))) return MODSX_ERR_NOMEM;
  }
  const size_t capExt = tap ? nExt : 0;
  if (tap && !c->sdExt.ensure(capExt * sizeof(SdExt) + 1)) return MODSX_ERR_NOMEM;
  const size_t capPts = c->sdPoints.cap / sizeof(SdPoint);
  std::vector<SdPoint> pts(nAcc);
  std::vector<SdExt> ext(capExt);
  if (nExt) {
    launch_surfdet_emit(c->stream, jobs, scanSegs, (int)pl.scanSegs.size(), pl.tiles, resp, lap, (const unsigned char *)c->sdFlags.p, offs,
                        (SdPoint *)c->sdPoints.p, (int)std::min<size_t>(capPts, 0x7fffffff), tap ? (SdExt *)c->sdExt.p : nullptr, (int)capExt);
    if (nAcc) MX_HIP(hipMemcpyAsync(pts.data(), c->sdPoints.p, nAcc * sizeof(SdPoint), hipMemcpyDeviceToHost, c->stream));
    if (capExt) MX_HIP(hipMemcpyAsync(ext.data(), c->sdExt.p, capExt * sizeof(SdExt), hipMemcpyDeviceToHost, c->stream));
  }
  if (tap) {      // one image
    const SdJob &J = pl.jobs[0];
    MX_HIP(hipMemcpyAsync(tap->integral, J.integ, (size_t)J.rows * J.cols * 4, hipMemcpyDeviceToHost, c->stream));
    MX_HIP(hipMemcpyAsync(tap->resp, c->sdResp.p, pl.planeValues * 4, hipMemcpyDeviceToHost, c->stream));
    MX_HIP(hipMemcpyAsync(tap->lap, c->sdLap.p, pl.planeValues, hipMemcpyDeviceToHost, c->stream));
    for (int k = 0; k < J.nLayers; k++) {
      tap->layers[4 * k] = J.L[k].w; tap->layers[4 * k + 1] = J.L[k].h; tap->layers[4 * k + 2] = J.L[k].step; tap->layers[4 * k + 3] = J.L[k].filter;
    }
  }
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  c->sdCounters[1] += n; c->sdCounters[2] += (long)nExt; c->sdCounters[3] += (long)nAcc;
  if (out)
    for (int j = 0; j < n; j++) {
      out[j].clear();
      out[j].reserve((size_t)(start[2 * (j + 1) + 1] - start[2 * j + 1]));
      for (int k = start[2 * j + 1]; k < start[2 * (j + 1) + 1]; k++) {
        modsx_keypoint kp;
        memset(&kp, 0, sizeof kp);       // the padding too: callers compare records as bytes
        kp.x = pts[k].x; kp.y = pts[k].y; kp.s = pts[k].scale;
        kp.a11 = cos(0.0); kp.a12 = sin(0.0); kp.a21 = -sin(0.0); kp.a22 = cos(0.0);
        out[j].push_back(kp);
      }
    }
  if (tap) {
    *tap->nExt = (int)nExt;
    for (size_t k = 0; k < nExt && (int)k < tap->capExt; k++) {
      const SdExt &e = ext[k];
      tap->ext[4 * k] = e.o; tap->ext[4 * k + 1] = e.i; tap->ext[4 * k + 2] = e.r; tap->ext[4 * k + 3] = e.c;
      memcpy(tap->dD + 3 * k, e.dD, sizeof e.dD); memcpy(tap->H + 6 * k, e.H, sizeof e.H); memcpy(tap->x + 3 * k, e.x, sizeof e.x);
      tap->accepted[k] = e.accepted; tap->laplacian[k] = e.laplacian;
    }
  }
  return MODSX_OK;
}

int detect_surf_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const modsx_surfdet_params &par, std::vector<modsx_keypoint> *out) {
  const modsx_surfdet_params p = surfdet_normalise(par);
  int rc = surfdet_check("modsx_detect_surf", imgs, n, p);
  if (rc) return rc;
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  c->sdCounters[0]++;
  for (int i0 = 0; i0 < n; i0 += MAXB)
    if ((rc = run_set(c, imgs + i0, std::min(MAXB, n - i0), p, out + i0, nullptr))) return rc;
  return MODSX_OK;
}

int debug_surfdet(modsx_ctx *c, const modsx_image *img, const modsx_surfdet_params &par, float *integral, int *layers, float *resp,
                  unsigned char *lap, int *ext, double *dD, double *H, double *x, int *accepted, int *laplacian, int capExt, int *nExt) {
  const modsx_surfdet_params p = surfdet_normalise(par);
  const modsx_image *imgs[1] = {img};
  int rc = surfdet_check("modsx_debug_surfdet", imgs, 1, p);
  if (rc) return rc;
  CtxBusy busy(c);
  c->sdCounters[0]++;
  const SurfdetTap tap = {integral, layers, resp, lap, ext, dD, H, x, accepted, laplacian, capExt, nExt};
  if ((rc = run_set(c, imgs, 1, p, nullptr, &tap))) return rc;
  return surfdet_geometry("modsx_debug_surfdet", img->rows, img->cols, p, nullptr);
}

}  // namespace mx
