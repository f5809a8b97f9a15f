// engine_caffe.hip -- the learned-descriptor front end: what the reference's "CAFFE" branch does around its network
// (imagerepresentation.cpp:1343-1534): the input blob of the regions of one image (caffe_patches) and the normalisation of the
// network's output rows (caffe_norm_rows, :181-217).  The contract is in include/modsx.h, the kernels are in kernels_caffe.hip.
//
// A patch call is one launch: the host fills one CaffeJob per region -- curr_sc (the f64 product rounded once), the six f32
// arguments interpolate() is called with and interpolateCheckBorders for them -- with caffe_jobs, the function modsx_caffe_jobs
// reports unchanged; the planes, the patch size and the truncated means travel as kernel arguments.  A workgroup is one region
// (caffe_geometry, engine.hpp: one lane per patch row, CAFFE_COLS columns per LDS tile).  A norm call is one launch over
// workgroups of CAFFE_NORM_ROWS rows; MODSX_CAFFE_NORM_NONE is a copy and launches nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

int caffe_check(const char *fn, const modsx_caffe_params &p) {
  const std::string f(fn);
  if (p.patchSize < 1 || p.patchSize > CAFFE_MAX_PATCH || p.patchSize % 2 == 0) {
    set_error(f + ": patchSize must be odd and in 1 .. 255 (interpolate overruns an even patch)");
    return MODSX_ERR_ARG;
  }
  if (!(std::isfinite(p.mrSize) && p.mrSize >= 0 && p.mrSize <= 1e6)) { set_error(f + ": mrSize must be finite and in 0 .. 1e6"); return MODSX_ERR_ARG; }
  for (int c = 0; c < 3; c++)
    if (!(std::isfinite(p.mean[c]) && fabs(p.mean[c]) <= 1073741824.0)) { set_error(f + ": a mean that is not finite or outside +-2^30"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

int caffe_norm_check(const char *fn, int n, int dim, int norm) {
  const std::string f(fn);
  if (n < 0) { set_error(f + ": bad argument"); return MODSX_ERR_ARG; }
  if (dim < 1 || dim > CAFFE_MAX_DIM) { set_error(f + ": dim must be in 1 .. 4096"); return MODSX_ERR_ARG; }
  if (norm < MODSX_CAFFE_NORM_L2 || norm > MODSX_CAFFE_NORM_NONE) { set_error(f + ": norm must be MODSX_CAFFE_NORM_L2, _L1, _ROOTL2 or _NONE"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

void caffe_jobs(const modsx_region *regs, int n, const modsx_caffe_params &p, int rows, int cols, CaffeJob *jobs) {
  const double mrScale = p.mrSize;                                                  // :1368
  const int patchImageSize = 2 * int(mrScale) + 1;                                  // :1369
  const double imageToPatchScale = double(patchImageSize) / (double)p.patchSize;    // :1370
  for (int i = 0; i < n; i++) {
    const modsx_keypoint &k = regs[i].reproj_kp;
    CaffeJob &j = jobs[i];
    j.sc = (float)(imageToPatchScale * k.s);                                        // :1395
    j.x = (float)k.x; j.y = (float)k.y;
    j.a11 = (float)k.a11 * j.sc; j.a12 = (float)k.a12 * j.sc; j.a21 = (float)k.a21 * j.sc; j.a22 = (float)k.a22 * j.sc;   // :1403-1406
    j.touch = check_borders_host(cols, rows, j.x, j.y, j.a11, j.a12, j.a21, j.a22, p.patchSize, p.patchSize) ? 1 : 0;
  }
}

static int plane_on_device(modsx_ctx *c, const char *fn, const float *p) {
  hipPointerAttribute_t at;
  const bool known = hipPointerGetAttributes(&at, p) == hipSuccess;
  if (!known) (void)hipGetLastError();
  if (!known || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
    set_error(std::string(fn) + ": a plane does not hold device memory");
    return MODSX_ERR_ARG;
  }
  if (at.device != c->dev) { set_error(std::string(fn) + ": a plane lives on another device than the context"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

int caffe_patches(modsx_ctx *c, const char *fn, const modsx_image *const *planes, int nplanes, const modsx_region *regs, int n,
                  const modsx_caffe_params &p, float *blob, bool onDevice, unsigned char *flags) {
  int rc = caffe_check(fn, p);
  if (rc) return rc;
  if (nplanes != 1 && nplanes != 3) { set_error(std::string(fn) + ": 1 (gray) or 3 (B, G, R) planes"); return MODSX_ERR_ARG; }
  for (int q = 1; q < nplanes; q++)
    if (planes[q]->rows != planes[0]->rows || planes[q]->cols != planes[0]->cols) {
      set_error(std::string(fn) + ": the planes have different sizes");
      return MODSX_ERR_ARG;
    }
  for (int q = 0; q < nplanes; q++)
    if ((rc = plane_on_device(c, fn, planes[q]->d))) return rc;
  if (n == 0) return MODSX_OK;
  const int P = p.patchSize, rows = planes[0]->rows, cols = planes[0]->cols;
  const size_t floats = (size_t)n * 3 * P * P;
  CtxBusy busy(c);
  if (!c->caffeJobs.ensure(sizeof(CaffeJob) * (size_t)n) || (flags && !c->caffeFlags.ensure((size_t)n)) ||
      (!onDevice && !c->caffeOut.ensure(floats * 4)))
    return MODSX_ERR_NOMEM;
  std::vector<CaffeJob> jobs(n);
  caffe_jobs(regs, n, p, rows, cols, jobs.data());
  long border = 0;
  for (const CaffeJob &j : jobs) border += j.touch;
  float *out = onDevice ? blob : (float *)c->caffeOut.p;
  unsigned char *dflags = flags ? (unsigned char *)c->caffeFlags.p : nullptr;
  MX_HIP(hipMemcpyAsync(c->caffeJobs.p, jobs.data(), sizeof(CaffeJob) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  launch_caffe_patches(c->stream, (const CaffeJob *)c->caffeJobs.p, n, planes[0]->d, planes[nplanes == 3 ? 1 : 0]->d,
                       planes[nplanes == 3 ? 2 : 0]->d, nplanes, rows, cols, P, (float)(int)p.mean[0], (float)(int)p.mean[1],
                       (float)(int)p.mean[2], out, dflags);
  hipError_t e = hipSuccess;
  if (!onDevice) e = hipMemcpyAsync(blob, out, floats * 4, hipMemcpyDeviceToHost, c->stream);
  if (flags && e == hipSuccess) e = hipMemcpyAsync(flags, dflags, (size_t)n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // pageable memory on the host side: the jobs are read by now
  if (e == hipSuccess) e = hipGetLastError();
  MX_HIP(e);
  c->caffeCounters[0]++;
  c->caffeCounters[1] += n;
  c->caffeCounters[2] += border;
  c->caffeCounters[3]++;
  return MODSX_OK;
}

int caffe_norm_rows(modsx_ctx *c, const char *fn, const float *rows, int n, int dim, int norm, float *out, bool onDevice) {
  const int rc = caffe_norm_check(fn, n, dim, norm);
  if (rc) return rc;
  if (n == 0) return MODSX_OK;
  const size_t bytes = (size_t)n * dim * 4;
  CtxBusy busy(c);
  if (onDevice) {
    if (norm == MODSX_CAFFE_NORM_NONE) {
      if (out != rows) MX_HIP(hipMemcpyAsync(out, rows, bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {
      launch_caffe_norm(c->stream, rows, n, dim, norm, out);
      c->caffeCounters[3]++;
    }
    MX_HIP(hipStreamSynchronize(c->stream));
    MX_HIP(hipGetLastError());
    return MODSX_OK;
  }
  if (!c->caffeOut.ensure(bytes)) return MODSX_ERR_NOMEM;
  float *d = (float *)c->caffeOut.p;
  MX_HIP(hipMemcpyAsync(d, rows, bytes, hipMemcpyHostToDevice, c->stream));
  if (norm != MODSX_CAFFE_NORM_NONE) { launch_caffe_norm(c->stream, d, n, dim, norm, d); c->caffeCounters[3]++; }
  MX_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

}  // namespace mx
