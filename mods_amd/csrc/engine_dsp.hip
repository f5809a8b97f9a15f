// engine_dsp.hip -- DSP-SIFT (domain-size pooling, imagerepresentation.cpp:1547-1598), its two halves as entries of their own.
//   * raw histograms: DescribeRegions<SIFTDescriptor{doNorm = false}> -- the description front end unchanged (windows, the chunk
//     planner, the sampling and blur launches of describe_batch) with the raw form of k_describe as the last launch (DescTail);
//   * the f32 norm: SIFTnorm(std::vector<float>&) over caller-supplied rows (kernels_dsp.hip);
//   * DSP-SIFT: numScales + 1 such passes at mrSize_k = mrSize * (startCoef + k * (endCoef - startCoef) / numScales), pass 0
//     storing and the later ones adding in f32 to the same [n][128] rows, then one norm launch in place.  The passes run on one
//     stream in order and each writes a region once, whatever the planner's cuts at that scale are, so the pooling order is the
//     reference's and the state is n x 512 bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>
#include <vector>
#include "describe_plan.hpp"

namespace mx {

constexpr int DSP_DIM = 128, DSP_MAX_SCALES = 64;
constexpr size_t DSP_ROW_B = (size_t)DSP_DIM * 4;

struct RawTail { float *out; int accumulate; };
static int tail_raw(modsx_ctx *c, void *self, const DescJob *jobs, int n, const float *grid, const int *needTab, const float *coordTab,
                    int photoNorm) {
  const RawTail *rt = (const RawTail *)self;
  launch_describe_raw(c->stream, jobs, n, (const ImgRef *)c->imgRefs.p, grid, needTab, coordTab, c->dSiftMask, c->dSiftMaskIdx,
                      c->nSiftMask, c->dSiftOTab, c->dSiftBins, c->dSiftW, photoNorm, rt->out, rt->accumulate,
                      c->dDescOrdered);
  return MODSX_OK;
}

// what describe_batch would refuse half way through a call (describe_size_plan), asked before anything is launched
static int check_windows(const char *fn, const modsx_region *regs, int n, double mrSize, int fast) {
  if (!(std::isfinite(mrSize) && mrSize > 0)) { set_error(std::string(fn) + ": a measurement size that is not finite and positive"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n; i++) {
    const int P = describe_window(regs[i].det_kp.s, mrSize, fast);
    if (P > 0 && blur_ksize(1.5f * (float(P - 2) / float(DESC_PATCH))) > 512) {
      set_error(std::string(fn) + ": descriptor window too large (blur kernel > 512 taps)");
      return MODSX_ERR_ARG;
    }
  }
  return MODSX_OK;
}

int describe_regions_raw(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize, int fast,
                         int photoNorm, float *hist, bool onDevice) {
  if (patchSize != DESC_PATCH) { set_error("modsx_describe_regions_raw: patchSize must be 41"); return MODSX_ERR_ARG; }
  if (n == 0) return MODSX_OK;
  int rc = check_windows("modsx_describe_regions_raw", regs, n, mrSize, fast);
  if (rc) return rc;
  CtxBusy busy(c);
  const size_t bytes = (size_t)n * DSP_ROW_B;
  RawTail rt = {hist, 0};
  if (!onDevice) { if (!c->dspRows.ensure(bytes)) return MODSX_ERR_NOMEM; rt.out = (float *)c->dspRows.p; }
  const std::vector<modsx_region> v(regs, regs + n);
  const DescTail tail = {tail_raw, &rt};
  if ((rc = describe_batch_tail(c, img, v, mrSize, patchSize, fast, photoNorm, tail))) return rc;
  if (!onDevice) MX_HIP(hipMemcpy(hist, rt.out, bytes, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

int sift_norm_rows(modsx_ctx *c, const float *rows, int n, double maxBinValue, float *out, bool onDevice) {
  if (n == 0) return MODSX_OK;
  CtxBusy busy(c);
  if (onDevice) {
    launch_sift_norm_f32(c->stream, rows, n, maxBinValue, out);
    MX_HIP(hipStreamSynchronize(c->stream));
    MX_HIP(hipGetLastError());
    return MODSX_OK;
  }
  const size_t bytes = (size_t)n * DSP_ROW_B;
  if (!c->dspRows.ensure(bytes)) return MODSX_ERR_NOMEM;
  float *d = (float *)c->dspRows.p;
  MX_HIP(hipMemcpyAsync(d, rows, bytes, hipMemcpyHostToDevice, c->stream));
  launch_sift_norm_f32(c->stream, d, n, maxBinValue, d);
  MX_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

int describe_regions_dspsift(modsx_ctx *c, const modsx_image *img, const modsx_region *regs, int n, double mrSize, int patchSize,
                             int fast, int photoNorm, int numScales, double startCoef, double endCoef, double maxBinValue, float *desc,
                             bool onDevice) {
  const char *fn = "modsx_describe_regions_dspsift";
  if (patchSize != DESC_PATCH) { set_error(std::string(fn) + ": patchSize must be 41"); return MODSX_ERR_ARG; }
  if (numScales < 1 || numScales > DSP_MAX_SCALES) { set_error(std::string(fn) + ": numScales must be 1..64"); return MODSX_ERR_ARG; }
  // curr_mrSize of imagerepresentation.cpp:1558-1559, in f64 as written: dsp_idx * (end_coef - start_coef) / num_domains is
  // (dsp_idx * (end_coef - start_coef)) / num_domains
  double mr[DSP_MAX_SCALES + 1];
  for (int k = 0; k <= numScales; k++) {
    mr[k] = mrSize * (startCoef + k * (endCoef - startCoef) / numScales);
    if (!(std::isfinite(mr[k]) && mr[k] > 0)) { set_error(std::string(fn) + ": a measurement size that is not finite and positive"); return MODSX_ERR_ARG; }
  }
  if (n == 0) return MODSX_OK;
  int rc;
  for (int k = 0; k <= numScales; k++)
    if ((rc = check_windows(fn, regs, n, mr[k], fast))) return rc;
  CtxBusy busy(c);
  const size_t bytes = (size_t)n * DSP_ROW_B;
  RawTail rt = {desc, 0};
  if (!onDevice) { if (!c->dspRows.ensure(bytes)) return MODSX_ERR_NOMEM; rt.out = (float *)c->dspRows.p; }
  const std::vector<modsx_region> v(regs, regs + n);
  const DescTail tail = {tail_raw, &rt};
  c->dspCounters[0]++; c->dspCounters[1] += n;
  for (int k = 0; k <= numScales; k++) {
    rt.accumulate = k > 0;
    if ((rc = describe_batch_tail(c, img, v, mr[k], patchSize, fast, photoNorm, tail))) return rc;
    c->dspCounters[2]++;
  }
  launch_sift_norm_f32(c->stream, rt.out, n, maxBinValue, rt.out);
  if (!onDevice) MX_HIP(hipMemcpyAsync(desc, rt.out, bytes, hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

}  // namespace mx
