/* TEST INFRASTRUCTURE ONLY.  This stands in for OpenCV's <opencv2/core/core.hpp> only so that three translation units of the
 * reference (detectors/helpers.cpp, matching/siftdesc.cpp, detectors/affinedetectors/affine.cpp, compiled in place by
 * oracle/Makefile into _ref/libhessaff_ref.so) parse and run.  They use cv::Mat as a CONTAINER and nothing else: rows, cols, step,
 * type(), ptr<T>, at<T>, the (rows, cols, type) constructor, copies that share the pixels, and `= cv::Scalar` (a fill).  That
 * container, the CV_32F type code and the MIN / MAX macros of OpenCV's C header are all that is DEFINED here.
 *
 * Every cv:: OPERATION the three files name -- GaussianBlur, SVD::compute, Mat_<float> << ..., Mat * Mat -- is only DECLARED: no
 * OpenCV arithmetic is restated in this directory.  They sit on branches the pinned entry points never take (gaussianBlur /
 * gaussianBlurInplace / doubleImage / halfImage callers, the AFF_BMBRG_HESSIAN branch of findAffineShape); oracle/ref_hessaff_shim.cpp
 * defines each of them as "print the name and abort" and refuses the parameters that would reach one.
 * <string> and <cmath> are here because the reference's headers use std::string and sqrt without including them. */
#ifndef MODSX_REF_STUB_MAT_OPENCV_CORE_HPP
#define MODSX_REF_STUB_MAT_OPENCV_CORE_HPP
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>

#define CV_32F 5
#define CV_32FC1 5
#ifndef MIN
#define MIN(a, b) ((a) > (b) ? (b) : (a))
#endif
#ifndef MAX
#define MAX(a, b) ((a) < (b) ? (b) : (a))
#endif

namespace cv {
struct Scalar {
  double v0;
  Scalar(double v = 0) : v0(v) {}
};
struct Size {
  int width, height;
  Size(int w, int h) : width(w), height(h) {}
};
enum { BORDER_REPLICATE = 1 };

/* rows x cols f32 pixels, rows `step` bytes apart; copies share the pixels, as OpenCV's header copies do */
struct Mat {
  int rows = 0, cols = 0;
  size_t step = 0;
  unsigned char *data = nullptr;
  Mat() {}
  Mat(int r, int c, int type) : rows(r), cols(c), step((size_t)c * sizeof(float)), type_(type) {
    const size_t n = (size_t)(r > 0 ? r : 0) * step;
    own_.reset(new unsigned char[n ? n : 1], std::default_delete<unsigned char[]>());
    memset(own_.get(), 0, n);
    data = own_.get();
  }
  int type() const { return type_; }
  template <typename T> T *ptr(int r = 0) { return (T *)(data + step * r); }
  template <typename T> const T *ptr(int r = 0) const { return (const T *)(data + step * r); }
  template <typename T> T &at(int r, int c) { return ((T *)(data + step * r))[c]; }
  template <typename T> const T &at(int r, int c) const { return ((const T *)(data + step * r))[c]; }
  Mat &operator=(const Scalar &s) {
    for (int r = 0; r < rows; r++)
      for (int c = 0; c < cols; c++) at<float>(r, c) = (float)s.v0;
    return *this;
  }

 private:
  int type_ = CV_32F;
  std::shared_ptr<unsigned char> own_;
};

/* ---- declared, never defined here (see the comment on top) ---- */
template <typename T> struct Mat_ : public Mat {
  Mat_(int rows, int cols);
};
template <typename T> struct MatCommaInitializer_ {
  MatCommaInitializer_ &operator,(T v);
  operator Mat() const;
};
template <typename T> MatCommaInitializer_<T> operator<<(const Mat_<T> &m, T v);
Mat operator*(const Mat &a, const Mat &b);
struct SVD {
  static void compute(const Mat &src, Mat &w, Mat &u, Mat &vt);
};
}  // namespace cv
#endif
