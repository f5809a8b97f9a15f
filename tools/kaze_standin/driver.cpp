// The driver of tools/make_kaze_fixture.py: C entries around the reference's AKAZE detector, compiled together with its
// akaze/src/lib/{AKAZE,nldiffusion_functions,fed}.cpp against the stand-in opencv2/ of this directory.
//   * the "KAZE" branch of imagerepresentation.cpp:678-681, 1132-1152 is restated: default AKAZEOptions with the image size, then
//     Create_Nonlinear_Scale_Space(pixels * 1.0 / 255.0) -- each f32 pixel times (float)(1.0 / 255.0) -- and Feature_Detection;
//   * this file alone sees the class with its private members opened (the layout is unchanged): it reads the level table, the tau
//     lists and the planes, and plants caller-supplied Ldet planes for the scan cases;
//   * what the reference keeps in locals is restated here from its compiled pieces and checked against its outputs: hmax and the
//     histogram of compute_k_percentile (the blur and the derivatives are the reference's own functions; the kcontrast the
//     fixture records is compute_k_percentile's return), the raw maxima of the 3 x 3 scan, and the list after the same-level /
//     lower-level pass (kaze_find asserts that the upper-level pass over that list gives Find_Scale_Space_Extrema's output);
//   * utils.cpp is not compiled (it needs highgui): convert_scale, which only Save_Scale_Space calls, aborts.
#include <bitset>
#include <fstream>
#include <iomanip>
#include <vector>
#include <opencv2/opencv.hpp>      // the system headers first: only AKAZE.h is read with private opened
#define private public
#include "AKAZE.h"
#undef private

void convert_scale(cv::Mat &) { abort(); }

namespace {
int fround(float flt) { return (int)(flt + 0.5f); }     // aka::fRound, which AKAZE.cpp keeps inline
struct Handle {
  aka::AKAZE *ak;
};
void put(const std::vector<cv::KeyPoint> &v, double *out, int cap) {
  for (size_t k = 0; k < v.size() && (int)k < cap; k++) {
    double *o = out + 6 * k;
    o[0] = v[k].pt.x; o[1] = v[k].pt.y; o[2] = v[k].size; o[3] = v[k].response; o[4] = v[k].octave; o[5] = v[k].class_id;
  }
}
}  // namespace

extern "C" {

void *kaze_new(int rows, int cols, int omax, int nsublevels, float soffset, float derivative_factor, float dthreshold,
               float min_dthreshold, float perc, int nbins, int descriptor) {
  aka::AKAZEOptions o;
  o.img_width = cols; o.img_height = rows;
  o.omax = omax; o.nsublevels = nsublevels; o.soffset = soffset; o.derivative_factor = derivative_factor;
  o.dthreshold = dthreshold; o.min_dthreshold = min_dthreshold; o.kcontrast_percentile = perc; o.kcontrast_nbins = (size_t)nbins;
  o.descriptor = (aka::DESCRIPTOR_TYPE)descriptor;
  Handle *h = new Handle;
  h->ak = new aka::AKAZE(o);
  return h;
}
void kaze_free(void *hv) { Handle *h = (Handle *)hv; delete h->ak; delete h; }

// table [n][6] = octave, sublevel, rows, cols, sigma_size, FED steps (0 for level 0); sig [n][2] = esigma, etime.  Returns n
int kaze_levels(void *hv, int *table, float *sig) {
  aka::AKAZE &a = *((Handle *)hv)->ak;
  for (size_t i = 0; i < a.evolution_.size(); i++) {
    const aka::TEvolution &e = a.evolution_[i];
    table[6 * i] = (int)e.octave; table[6 * i + 1] = (int)e.sublevel; table[6 * i + 2] = e.Lt.rows; table[6 * i + 3] = e.Lt.cols;
    table[6 * i + 4] = (int)e.sigma_size; table[6 * i + 5] = i ? a.nsteps_[i - 1] : 0;
    sig[2 * i] = e.esigma; sig[2 * i + 1] = e.etime;
  }
  return (int)a.evolution_.size();
}
int kaze_omax(void *hv) { return ((Handle *)hv)->ak->options_.omax; }
int kaze_tau(void *hv, int level, float *out) {
  aka::AKAZE &a = *((Handle *)hv)->ak;
  if (level < 1 || level > (int)a.tsteps_.size()) return 0;
  const std::vector<float> &t = a.tsteps_[level - 1];
  for (size_t k = 0; k < t.size(); k++) out[k] = t[k];
  return (int)t.size();
}

// the scale space of the view; kc [3] = compute_k_percentile's return, hmax, options_.kcontrast afterwards; hist [nbins] counts
int kaze_create(void *hv, const float *pixels, float *kc, long *hist) {
  aka::AKAZE &a = *((Handle *)hv)->ak;
  const int rows = a.options_.img_height, cols = a.options_.img_width, nbins = (int)a.options_.kcontrast_nbins;
  cv::Mat img(rows, cols, CV_32F);
  const float scale = (float)(1.0 / 255.0);
  for (size_t i = 0; i < (size_t)rows * cols; i++) img.ptr<float>(0)[i] = pixels[i] * scale;
  kc[0] = compute_k_percentile(img, a.options_.kcontrast_percentile, 1.0, a.options_.kcontrast_nbins, 0, 0);
  {
    cv::Mat g = cv::Mat::zeros(rows, cols, CV_32F), Lx = cv::Mat::zeros(rows, cols, CV_32F), Ly = cv::Mat::zeros(rows, cols, CV_32F);
    gaussian_2D_convolution(img, g, 0, 0, 1.0);
    image_derivatives_scharr(g, Lx, 1, 0);
    image_derivatives_scharr(g, Ly, 0, 1);
    float hmax = 0.0f;
    for (int pass = 0; pass < 2; pass++)
      for (int i = 1; i < rows - 1; i++)
        for (int j = 1; j < cols - 1; j++) {
          const float lx = Lx.ptr<float>(i)[j], ly = Ly.ptr<float>(i)[j];
          const float m = sqrtf(lx * lx + ly * ly);
          if (pass == 0) { if (m > hmax) hmax = m; }
          else if (m != 0.0f) {
            size_t b = (size_t)floorf((float)nbins * (m / hmax));
            if (b == (size_t)nbins) b--;
            hist[b]++;
          }
        }
    kc[1] = hmax;
  }
  const int rc = a.Create_Nonlinear_Scale_Space(img);
  kc[2] = a.options_.kcontrast;
  return rc;
}

// which: 0 Lt, 1 Lsmooth, 2 Lflow, 3 Ldet
int kaze_plane(void *hv, int level, int which, float *out) {
  aka::AKAZE &a = *((Handle *)hv)->ak;
  const aka::TEvolution &e = a.evolution_[level];
  const cv::Mat &m = which == 0 ? e.Lt : which == 1 ? e.Lsmooth : which == 2 ? e.Lflow : e.Ldet;
  if (m.empty() || m.rows != e.Lt.rows || m.cols != e.Lt.cols) return -1;
  memcpy(out, m.ptr<float>(0), (size_t)m.rows * m.cols * 4);
  return 0;
}
void kaze_response(void *hv) { ((Handle *)hv)->ak->Compute_Determinant_Hessian_Response(); }
void kaze_plant(void *hv, int level, const float *plane) {
  cv::Mat &m = ((Handle *)hv)->ak->evolution_[level].Ldet;
  memcpy(m.ptr<float>(0), plane, (size_t)m.rows * m.cols * 4);
}

// Find_Scale_Space_Extrema and Do_Subpixel_Refinement on the Ldet planes the object holds.  raw [capRaw][3] = level, row, col and
// rawv their values; aux, upper, final [cap][6] = x, y, size, response, octave, class_id.  counts [4]; returns 0, -1 where a buffer
// is too small, -2 where the restated passes disagree with the reference's output.
int kaze_find(void *hv, int *raw, float *rawv, int capRaw, double *aux, double *upper, double *fin, int cap, long *counts) {
  Handle *h = (Handle *)hv;
  aka::AKAZE &a = *h->ak;
  const aka::AKAZEOptions &op = a.options_;
  float smax = 0.0f;
  if (op.descriptor == aka::SURF_UPRIGHT || op.descriptor == aka::SURF || op.descriptor == aka::MLDB_UPRIGHT || op.descriptor == aka::MLDB)
    smax = 10.0 * sqrtf(2.0);
  else if (op.descriptor == aka::MSURF_UPRIGHT || op.descriptor == aka::MSURF)
    smax = 12.0 * sqrtf(2.0);
  std::vector<cv::KeyPoint> A;
  long nraw = 0;
  for (size_t i = 0; i < a.evolution_.size(); i++) {
    const cv::Mat &L = a.evolution_[i].Ldet;
    for (int r = 1; r < L.rows - 1; r++)
      for (int c = 1; c < L.cols - 1; c++) {
        const float *p = L.ptr<float>(r) + c, *u = L.ptr<float>(r - 1) + c, *d = L.ptr<float>(r + 1) + c;
        const float v = *p;
        if (!(v > op.dthreshold && v >= op.min_dthreshold && v > p[-1] && v > p[1] && v > u[-1] && v > u[0] && v > u[1] && v > d[-1] &&
              v > d[0] && v > d[1]))
          continue;
        if (nraw < capRaw) { raw[3 * nraw] = (int)i; raw[3 * nraw + 1] = r; raw[3 * nraw + 2] = c; rawv[nraw] = v; }
        nraw++;
        cv::KeyPoint pt;
        pt.response = fabs(v);
        pt.size = a.evolution_[i].esigma * op.derivative_factor;
        pt.octave = (int)a.evolution_[i].octave;
        pt.class_id = (int)i;
        const float ratio = pow(2.f, pt.octave);
        const int ss = fround(pt.size / ratio);
        pt.pt.x = c; pt.pt.y = r;
        bool keep = true, repeated = false;
        size_t id = 0;
        for (size_t k = 0; k < A.size(); k++)
          if (pt.class_id - 1 == A[k].class_id || pt.class_id == A[k].class_id) {
            const float dist = sqrt(pow(pt.pt.x * ratio - A[k].pt.x, 2) + pow(pt.pt.y * ratio - A[k].pt.y, 2));
            if (dist <= pt.size) {
              if (pt.response > A[k].response) { id = k; repeated = true; } else keep = false;
              break;
            }
          }
        if (!keep) continue;
        const int lx = fround(pt.pt.x - smax * ss) - 1, rx = fround(pt.pt.x + smax * ss) + 1,
                  uy = fround(pt.pt.y - smax * ss) - 1, dy = fround(pt.pt.y + smax * ss) + 1;
        if (lx < 0 || rx >= L.cols || uy < 0 || dy >= L.rows) continue;
        pt.pt.x *= ratio; pt.pt.y *= ratio;
        if (repeated) A[id] = pt; else A.push_back(pt);
      }
  }
  std::vector<cv::KeyPoint> U;
  for (size_t i = 0; i < A.size(); i++) {
    bool repeated = false;
    for (size_t j = i + 1; j < A.size() && !repeated; j++)
      if (A[i].class_id + 1 == A[j].class_id) {
        const float dist = sqrt(pow(A[i].pt.x - A[j].pt.x, 2) + pow(A[i].pt.y - A[j].pt.y, 2));
        if (dist <= A[i].size && A[i].response < A[j].response) repeated = true;
      }
    if (!repeated) U.push_back(A[i]);
  }
  std::vector<cv::KeyPoint> ref;
  a.Find_Scale_Space_Extrema(ref);
  int rc = 0;
  if (ref.size() != U.size()) rc = -2;
  for (size_t k = 0; k < ref.size() && rc == 0; k++)
    if (ref[k].pt.x != U[k].pt.x || ref[k].pt.y != U[k].pt.y || ref[k].size != U[k].size || ref[k].response != U[k].response ||
        ref[k].octave != U[k].octave || ref[k].class_id != U[k].class_id)
      rc = -2;
  std::vector<cv::KeyPoint> F = ref;
  a.Do_Subpixel_Refinement(F);
  counts[0] = nraw; counts[1] = (long)A.size(); counts[2] = (long)ref.size(); counts[3] = (long)F.size();
  put(A, aux, cap); put(ref, upper, cap); put(F, fin, cap);
  if (rc == 0 && (nraw > capRaw || (long)A.size() > cap)) rc = -1;
  return rc;
}

}
