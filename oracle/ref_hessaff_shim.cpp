/* TEST INFRASTRUCTURE ONLY.  C entry points of oracle/_ref/libhessaff_ref.so: the reference's own detectors/helpers.cpp,
 * matching/siftdesc.cpp and detectors/affinedetectors/affine.cpp, compiled in place from $(REF) (oracle/Makefile) against the
 * stand-in cv::Mat of oracle/ref_stub_mat/.  Everything below is this project's text; every number an entry returns is computed by
 * the reference's functions, called the way its own callers do (DescribeRegions, synth-detection.hpp:169-255; AffineDetector,
 * scale-space-detector.cpp; DetectAffineShape, synth-detection.cpp:922-1074).
 *
 * The cv:: operations the three files name are defined here as "print the name and abort": no pinned entry reaches one.  What
 * would is refused with an error return instead (REFHESS_REFUSED): affBmbrgMethod != AFF_BMBRG_SMM (cv::Mat_ <<, SVD::compute,
 * Mat * Mat); gaussianBlur, gaussianBlurInplace, doubleImage and halfImage have no entry at all (cv::GaussianBlur, and doubleImage
 * indexes with Mat::step as a pixel count).
 *
 * Also refused, because the reference itself reads or writes out of bounds there:
 *   - atan2LUTff (helpers.cpp:160-207) casts 255 * q to int with no range check: a NaN operand, two infinities, or an operand so
 *     large that 255.f * it overflows index ATAN_LUT far outside its 256 entries.  Entries that run it (atan2, sift, grad_mag_ori)
 *     refuse such operands (`lut_safe`);
 *   - interpolate (helpers.cpp:551-626) writes (2 (cols >> 1) + 1) x (2 (rows >> 1) + 1) pixels, so an even result size overruns the
 *     result, and its unchecked branch casts NaN coordinates to int: even sizes and non-finite parameters are refused;
 *   - computeGaussMask (helpers.cpp:411-440) writes index `size` of an even-sized mask: even SMM windows are refused;
 *   - SIFTDescriptor::SIFTnorm(vector<double>&) (siftdesc.cpp:247-262) runs its clip loop to the MEMBER vec.size() = 128 on the
 *     64-element HalfSIFT vector inside operator() (siftdesc.cpp:417-430): 64 doubles read, and written where they exceed
 *     maxBinValue, behind a heap block.  HalfSIFT (type 2) therefore never goes through operator() here (route 0 refuses it).
 *     Route 1 takes the reference's raw histogram (operator() with doNorm = false), folds it HERE the way siftdesc.cpp:419-425
 *     does and hands the reference's public SIFTnorm / RootSIFTnorm a 64-element vector that owns 128 zeroed doubles, so that the
 *     over-long loop reads zeros and writes nothing.  HalfRootSIFT (type 3) runs through both routes (RootSIFTnorm loops over its
 *     argument's own size); tests/test_ref_pin_cpu.py requires the two routes to agree on every patch, which ties the fold here
 *     to the reference's.
 */
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "affinedetectors/affine.h"
#include "helpers.h"
#include "siftdesc.h"
#include <opencv2/imgproc/imgproc.hpp>

static void die(const char *name) {
  fprintf(stderr, "libhessaff_ref: %s was reached -- it is declared for parsing only (oracle/ref_stub_mat)\n", name);
  abort();
}

namespace cv {
void GaussianBlur(const Mat &, Mat &, Size, double, double, int) { die("cv::GaussianBlur"); }
Mat operator*(const Mat &, const Mat &) { die("cv::operator*(Mat, Mat)"); return Mat(); }
void SVD::compute(const Mat &, Mat &, Mat &, Mat &) { die("cv::SVD::compute"); }
template <> Mat_<float>::Mat_(int, int) { die("cv::Mat_<float>::Mat_"); }
template <> MatCommaInitializer_<float> &MatCommaInitializer_<float>::operator,(float) { die("cv::MatCommaInitializer_::operator,"); return *this; }
template <> MatCommaInitializer_<float>::operator Mat() const { die("cv::MatCommaInitializer_::operator Mat"); return Mat(); }
template <> MatCommaInitializer_<float> operator<<(const Mat_<float> &, float) { die("cv::operator<<(Mat_, float)"); return MatCommaInitializer_<float>(); }
}  // namespace cv

enum { REFHESS_REFUSED = -2 };

static cv::Mat mat_of(const float *src, int rows, int cols) {
  cv::Mat m(rows, cols, CV_32FC1);
  if (src) memcpy(m.data, src, (size_t)rows * cols * sizeof(float));
  return m;
}
/* a header over the caller's pixels, for images the reference only reads */
static cv::Mat view_of(const float *src, int rows, int cols) {
  cv::Mat m;
  m.rows = rows;
  m.cols = cols;
  m.step = (size_t)cols * sizeof(float);
  m.data = (unsigned char *)src;
  return m;
}
static void mat_out(const cv::Mat &m, float *dst) { memcpy(dst, m.data, (size_t)m.rows * m.cols * sizeof(float)); }

/* operands atan2LUTff can be handed without indexing outside ATAN_LUT (see the comment on top) */
static bool lut_operand_safe(float v) { return std::isinf(v) || std::fabs(v) <= FLT_MAX / 256.0f; }
static bool lut_safe(float y, float x) {
  if (std::isnan(x) || std::isnan(y) || (std::isinf(x) && std::isinf(y))) return false;
  return lut_operand_safe(x) && lut_operand_safe(y);
}
/* an image whose central / one-sided differences are all lut_safe */
static bool gradients_lut_safe(const float *p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!(std::fabs(p[i]) <= FLT_MAX / 1024.0f)) return false;
  return true;
}
static bool all_finite(const float *p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}

struct ShapeCatcher : public AffineShapeCallback {
  int hits = 0, iters = -1;
  float u[4] = {0, 0, 0, 0};
  void onAffineShapeFound(const cv::Mat &, float, float, float, float, float a11, float a12, float a21, float a22, int, float,
                          int it) override {
    hits++;
    u[0] = a11; u[1] = a12; u[2] = a21; u[3] = a22;
    iters = it;
  }
};

extern "C" {

float refhess_atan2lutff(float y, float x, int *refused) {
  *refused = lut_safe(y, x) ? 0 : 1;
  return *refused ? 0.f : atan2LUTff(y, x);
}

/* SIFTDescriptor on a 41 x 41 patch (the caller normalises it first when it wants DescribeRegions' photoNorm).  desc_type: 0 SIFT,
 * 1 RootSIFT, 2 HalfSIFT, 3 HalfRootSIFT; route 0 = operator() as DescribeRegions calls it, route 1 = the fold route described on
 * top (types 2 and 3).  desc: 128 floats, a Half type fills 64 and zeroes the rest.  raw: the public `vec` after operator() with
 * doNorm = false (128 doubles).  Returns the descriptor's length. */
int refhess_sift(const float *patch41, int desc_type, double max_bin, int route, float *desc, double *raw) {
  if (desc_type < 0 || desc_type > 3 || route < 0 || route > 1) return REFHESS_REFUSED;
  if (route == 0 && desc_type == 2) return REFHESS_REFUSED;
  if (route == 1 && desc_type < 2) return REFHESS_REFUSED;
  if (!gradients_lut_safe(patch41, 41 * 41)) return REFHESS_REFUSED;
  SIFTDescriptorParams par;
  par.maxBinValue = max_bin;
  par.useRootSIFT = (desc_type & 1) ? 1 : 0;
  std::vector<float> out;
  {
    SIFTDescriptorParams praw = par;
    praw.doNorm = false;
    SIFTDescriptor sift(praw);
    cv::Mat patch = mat_of(patch41, 41, 41);
    sift(patch, out);
    for (int i = 0; i < 128; i++) raw[i] = sift.vec[i];
  }
  if (route == 0) {
    par.doHalfSIFT = desc_type >= 2 ? 1 : 0;
    SIFTDescriptor sift(par);
    cv::Mat patch = mat_of(patch41, 41, 41);
    sift(patch, out);
  } else {
    SIFTDescriptor sift(par);
    std::vector<double> half(128, 0.0);
    half.resize(64);                      /* 64 elements on storage that holds 128 zeroed doubles */
    for (int i = 0, b = 0; i < 16; i++)
      for (int j = 0; j < 4; j++) half[b++] = raw[i * 8 + j] + raw[i * 8 + j + 4];
    if (desc_type & 1) sift.RootSIFTnorm(half);
    else sift.SIFTnorm(half);
    out.resize(64);
    for (int i = 0; i < 64; i++) out[i] = (float)half[i];
  }
  for (int i = 0; i < 128; i++) desc[i] = i < (int)out.size() ? out[i] : 0.f;
  return (int)out.size();
}

/* photometricallyNormalize in place; mask == NULL: computeCircularGaussMask(mask) of the patch's size, as DescribeRegions builds it */
int refhess_photo_norm(float *patch, int rows, int cols, const float *mask, float *sum, float *var) {
  if (rows < 1 || cols < 1) return REFHESS_REFUSED;
  cv::Mat p = mat_of(patch, rows, cols), m = mat_of(mask, rows, cols);
  if (!mask) computeCircularGaussMask(m);
  photometricallyNormalize(p, m, *sum, *var);
  mat_out(p, patch);
  return 0;
}

int refhess_circular_gauss_mask(int rows, int cols, float sigma, float *out) {
  if (rows < 1 || cols < 1) return REFHESS_REFUSED;
  cv::Mat m(rows, cols, CV_32FC1);
  computeCircularGaussMask(m, sigma);
  mat_out(m, out);
  return 0;
}

int refhess_gauss_mask(int size, float *out) {
  if (size < 1 || (size & 1) == 0) return REFHESS_REFUSED;
  cv::Mat m(size, size, CV_32FC1);
  computeGaussMask(m);
  mat_out(m, out);
  return 0;
}

/* interpolate: returns its bool, res = rrows x rcols */
int refhess_interpolate(const float *im, int rows, int cols, float ofsx, float ofsy, float a11, float a12, float a21, float a22,
                        float *res, int rrows, int rcols) {
  const float par[6] = {ofsx, ofsy, a11, a12, a21, a22};
  if (rows < 1 || cols < 1 || rrows < 1 || rcols < 1 || !(rrows & 1) || !(rcols & 1) || !all_finite(par, 6)) return REFHESS_REFUSED;
  const cv::Mat src = view_of(im, rows, cols);
  cv::Mat dst(rrows, rcols, CV_32FC1);
  const bool t = interpolate(src, ofsx, ofsy, a11, a12, a21, a22, dst);
  mat_out(dst, res);
  return t ? 1 : 0;
}

int refhess_check_borders(int orig_w, int orig_h, float ofsx, float ofsy, float a11, float a12, float a21, float a22, int res_w,
                          int res_h) {
  return interpolateCheckBorders(orig_w, orig_h, ofsx, ofsy, a11, a12, a21, a22, res_w, res_h) ? 1 : 0;
}

/* the cv::Mat overload: only the sizes of the two Mats are read */
int refhess_check_borders_mat(int rows, int cols, float ofsx, float ofsy, float a11, float a12, float a21, float a22, int rrows,
                              int rcols) {
  cv::Mat im, res;
  im.rows = rows; im.cols = cols;
  res.rows = rrows; res.cols = rcols;
  return interpolateCheckBorders(im, ofsx, ofsy, a11, a12, a21, a22, res) ? 1 : 0;
}

void refhess_inv_sqrt(float *abc, float *l12) { invSqrt(abc[0], abc[1], abc[2], l12[0], l12[1]); }

int refhess_get_eigenvalues(float a, float b, float c, float d, float *l12) { return getEigenvalues(a, b, c, d, l12[0], l12[1]) ? 1 : 0; }

void refhess_solve_linear3x3(float *A9, float *b3) { solveLinear3x3(A9, b3); }

/* the three overloads of rectifyAffineTransformationUpIsUp: float references, double references, double pointer */
void refhess_rectify_f(float *a) { rectifyAffineTransformationUpIsUp(a[0], a[1], a[2], a[3]); }
void refhess_rectify_d(double *a) { rectifyAffineTransformationUpIsUp(a[0], a[1], a[2], a[3]); }
void refhess_rectify_dp(double *a) { rectifyAffineTransformationUpIsUp(a); }

int refhess_compute_gradient(const float *img, int rows, int cols, float *gx, float *gy) {
  if (rows < 2 || cols < 2) return REFHESS_REFUSED;      /* the one-sided differences read column 1 / row 1 */
  cv::Mat m = mat_of(img, rows, cols), x(rows, cols, CV_32FC1), y(rows, cols, CV_32FC1);
  computeGradient(m, x, y);
  mat_out(x, gx);
  mat_out(y, gy);
  return 0;
}

/* interior pixels only, as the reference writes them; the frame of mag and ori comes back 0 */
int refhess_grad_mag_ori(const float *img, int rows, int cols, float *mag, float *ori) {
  if (rows < 1 || cols < 1 || !gradients_lut_safe(img, (size_t)rows * cols)) return REFHESS_REFUSED;
  cv::Mat m = mat_of(img, rows, cols), g(rows, cols, CV_32FC1), o(rows, cols, CV_32FC1);
  computeGradientMagnitudeAndOrientation(m, g, o);
  mat_out(g, mag);
  mat_out(o, ori);
  return 0;
}

/* AffineShape::findAffineShape over a job list, through an AffineShapeCallback: job k reads planes[plane_of[k]] at xyspd[4k ..] =
 * x, y, s, pixelDistance.  hit[k] = its return value (the callback ran exactly then); u and iters are what the callback was
 * handed, written for hits only -- the reference reports nothing about a keypoint that did not converge.  Returns n. */
int refhess_find_affine_shape_batch(const float *const *planes, const int *rows, const int *cols, int nplanes, const int *plane_of,
                                    const float *xyspd, int n, int maxIterations, float convergenceThreshold, int smmWindowSize,
                                    float initialSigma, int doBaumberg, int affBmbrgMethod, int *hit, float *u, int *iters) {
  if (affBmbrgMethod != AFF_BMBRG_SMM) return REFHESS_REFUSED;
  if (smmWindowSize < 3 || (smmWindowSize & 1) == 0 || !(initialSigma > 0) || !std::isfinite(initialSigma)) return REFHESS_REFUSED;
  if (!all_finite(xyspd, (size_t)4 * n)) return REFHESS_REFUSED;
  for (int k = 0; k < n; k++)
    if (plane_of[k] < 0 || plane_of[k] >= nplanes || !(xyspd[4 * k + 3] > 0)) return REFHESS_REFUSED;
  AffineShapeParams par;
  par.maxIterations = maxIterations;
  par.convergenceThreshold = convergenceThreshold;
  par.smmWindowSize = smmWindowSize;
  par.initialSigma = initialSigma;
  par.doBaumberg = doBaumberg;
  par.affBmbrgMethod = AFF_BMBRG_SMM;
  AffineShape shape(par);
  std::vector<cv::Mat> im;
  for (int i = 0; i < nplanes; i++) {
    if (rows[i] < 1 || cols[i] < 1 || !all_finite(planes[i], (size_t)rows[i] * cols[i])) return REFHESS_REFUSED;
    im.push_back(view_of(planes[i], rows[i], cols[i]));
  }
  for (int k = 0; k < n; k++) {
    ShapeCatcher got;
    shape.setAffineShapeCallback(&got);
    const float *q = xyspd + 4 * (size_t)k;
    const bool ok = shape.findAffineShape(im[plane_of[k]], q[0], q[1], q[2], q[3], 0, 0.f);
    if ((ok ? 1 : 0) != got.hits) return -3;               /* the callback runs exactly when it returns true */
    hit[k] = ok ? 1 : 0;
    if (ok) {
      memcpy(u + 4 * (size_t)k, got.u, sizeof got.u);
      iters[k] = got.iters;
    }
  }
  return n;
}
}
