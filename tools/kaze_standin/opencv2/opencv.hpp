// A stand-in for <opencv2/opencv.hpp>, just wide enough for tools/make_kaze_fixture.py to compile the reference's
// akaze/src/lib/{AKAZE,nldiffusion_functions,fed}.cpp without OpenCV.  It is the one place where the arithmetic of the OpenCV
// calls those sources make is specified (include/modsx.h restates the rules; none of them is pinned against a real OpenCV):
//   * GaussianBlur(f32, BORDER_REPLICATE): the library's gaussian_kernel(n, sigma) (cv::getGaussianKernel: taps from exp() in
//     f64, stored f32, normalised by the f64 sum of the f32 taps), a row pass (n <= 5: centre product first, then (left + right)
//     * tap outwards; else taps in ascending order from 0.f) and a symmetric column pass tap[R] * centre + 0.f, then
//     tap[R + j] * (below + above);
//   * Scharr / sepFilter2D (f32, BORDER_REFLECT_101): a row pass into an f32 plane, then a column pass; taps in ascending index
//     order, every product and every add rounded to f32, starting from the first product;
//   * Mat expressions: element-wise f32 operations, each rounded; X / s is X * (float)(1.0 / (double)s), s + X and s - X are f32
//     adds of (float)s, s / X is an IEEE f32 division, X * s a multiply by (float)s;
//   * resize(INTER_AREA): (((a + b) + c) + d) * 0.25f where both ratios are exactly 2, otherwise the area table (see resize);
//   * solve(2 x 2, DECOMP_LU): Cramer's rule in f64 with one reciprocal; dst is left alone where the determinant is 0.
// Everything not named here either stores bytes (Mat, Mat_, KeyPoint) or aborts (convertTo, imwrite).  Not OpenCV and not for
// anything else.
#pragma once
#include <assert.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_8UC1 0
#define CV_32S 4
#define CV_32F 5
#define CV_32FC1 5
#define CV_PI 3.1415926535897932384626433832795

namespace cv {

enum { BORDER_REPLICATE = 1, BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4 };
enum { INTER_AREA = 3 };
enum { DECOMP_LU = 0 };

struct Size { int width, height; Size() : width(0), height(0) {} Size(int w, int h) : width(w), height(h) {} };
template <typename T> struct Point_ { T x, y; Point_() : x(0), y(0) {} Point_(T a, T b) : x(a), y(b) {} };
typedef Point_<float> Point2f;
struct KeyPoint {
  Point2f pt; float size, angle, response; int octave, class_id;
  KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
};
struct DMatch { int queryIdx, trainIdx, imgIdx; float distance; };

inline size_t elem_size(int type) { return type == CV_8U ? 1 : 4; }

class Mat {
 public:
  int rows, cols, tp;
  std::shared_ptr<std::vector<unsigned char> > buf;
  size_t ofs;
  Mat() : rows(0), cols(0), tp(CV_32F), ofs(0) {}
  Mat(int r, int c, int type) : ofs(0) { create(r, c, type); }
  Mat(int r, int c, int type, void *data) : ofs(0) { create(r, c, type); memcpy(raw(), data, bytes()); }   // a copy: only ever read
  void create(int r, int c, int type) {
    if (buf && r == rows && c == cols && type == tp) return;
    rows = r; cols = c; tp = type; ofs = 0;
    buf = std::make_shared<std::vector<unsigned char> >((size_t)r * c * elem_size(type), (unsigned char)0);
  }
  static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
  size_t bytes() const { return (size_t)rows * cols * elem_size(tp); }
  unsigned char *raw() const { return buf ? buf->data() + ofs : 0; }
  template <typename T> T *ptr(int r = 0) { return (T *)raw() + (size_t)r * cols; }
  template <typename T> const T *ptr(int r = 0) const { return (const T *)raw() + (size_t)r * cols; }
  Size size() const { return Size(cols, rows); }
  bool empty() const { return !buf || rows * cols == 0; }
  void copyTo(Mat &dst) const {
    if (!(dst.buf && dst.rows == rows && dst.cols == cols && dst.tp == tp)) { dst = Mat(); dst.create(rows, cols, tp); }
    if (dst.raw() != raw()) memmove(dst.raw(), raw(), bytes());
  }
  Mat clone() const { Mat m; copyTo(m); return m; }
  Mat rowRange(int a, int b) const { Mat m = *this; m.rows = b - a; m.ofs = ofs + (size_t)a * cols * elem_size(tp); return m; }
  Mat row(int k) const { return rowRange(k, k + 1); }
  Mat mul(const Mat &o) const;
  void convertTo(Mat &, int, double = 1, double = 0) const { abort(); }
};

template <typename T> class Mat_ : public Mat {
 public:
  Mat_() {}
  Mat_(int r, int c) : Mat(r, c, sizeof(T) == 1 ? CV_8U : (T(0.5) == T(0) ? CV_32S : CV_32F)) {}
  Mat_(const Mat &m) : Mat(m) {}
  static Mat_<T> zeros(int r, int c) { return Mat_<T>(r, c); }
  T &operator()(int r, int c) { return ptr<T>(r)[c]; }
  Mat_<T> &operator=(const T &v) { T *p = ptr<T>(0); for (size_t i = 0; i < (size_t)rows * cols; i++) p[i] = v; return *this; }
};

// element-wise f32 operations, each rounded
template <typename F> inline Mat map1(const Mat &a, F f) {
  assert(a.tp == CV_32F);
  Mat o(a.rows, a.cols, CV_32F);
  const float *A = a.ptr<float>(0); float *O = o.ptr<float>(0);
  for (size_t i = 0; i < (size_t)a.rows * a.cols; i++) O[i] = f(A[i]);
  return o;
}
template <typename F> inline Mat map2(const Mat &a, const Mat &b, F f) {
  assert(a.tp == CV_32F && b.tp == CV_32F && a.rows == b.rows && a.cols == b.cols);
  Mat o(a.rows, a.cols, CV_32F);
  const float *A = a.ptr<float>(0), *B = b.ptr<float>(0); float *O = o.ptr<float>(0);
  for (size_t i = 0; i < (size_t)a.rows * a.cols; i++) O[i] = f(A[i], B[i]);
  return o;
}
struct op_add { float operator()(float a, float b) const { return a + b; } };
struct op_sub { float operator()(float a, float b) const { return a - b; } };
struct op_mul { float operator()(float a, float b) const { return a * b; } };
struct op_scale { float s; float operator()(float a) const { return a * s; } };
struct op_sadd { float s; float operator()(float a) const { return s + a; } };
struct op_ssub { float s; float operator()(float a) const { return s - a; } };
struct op_sdiv { float s; float operator()(float a) const { return s / a; } };
struct op_neg { float operator()(float a) const { return -a; } };
struct op_exp { float operator()(float a) const { return expf(a); } };
struct op_sqrt { float operator()(float a) const { return sqrtf(a); } };
struct op_pow { double p; float operator()(float a) const { return (float)::pow((double)a, p); } };
inline Mat Mat::mul(const Mat &o) const { return map2(*this, o, op_mul()); }
inline Mat operator+(const Mat &a, const Mat &b) { return map2(a, b, op_add()); }
inline Mat operator-(const Mat &a, const Mat &b) { return map2(a, b, op_sub()); }
inline Mat operator-(const Mat &a) { return map1(a, op_neg()); }
inline Mat operator*(const Mat &a, double s) { op_scale f = {(float)s}; return map1(a, f); }
inline Mat operator/(const Mat &a, double s) { op_scale f = {(float)(1.0 / s)}; return map1(a, f); }
inline Mat operator+(double s, const Mat &a) { op_sadd f = {(float)s}; return map1(a, f); }
inline Mat operator-(double s, const Mat &a) { op_ssub f = {(float)s}; return map1(a, f); }
inline Mat operator/(double s, const Mat &a) { op_sdiv f = {(float)s}; return map1(a, f); }
inline void exp(const Mat &a, Mat &dst) { dst = map1(a, op_exp()); }
inline void sqrt(const Mat &a, Mat &dst) { dst = map1(a, op_sqrt()); }
inline void pow(const Mat &a, double p, Mat &dst) { op_pow f = {p}; dst = map1(a, f); }

class _OutputArray {
 public:
  Mat *m;
  _OutputArray(Mat &mm) : m(&mm) {}
  void create(int r, int c, int type, int = -1, bool = false) const { *m = Mat(r, c, type); }
  Mat getMat() const { return *m; }
};
typedef const _OutputArray &OutputArray;

inline long getTickCount() { return 0; }
inline double getTickFrequency() { return 1.0; }
inline bool imwrite(const std::string &, const Mat &) { abort(); return false; }

inline int border_replicate(int p, int n) { return p < 0 ? 0 : (p > n - 1 ? n - 1 : p); }
inline int border_reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; }
  return p;
}

inline std::vector<float> gaussian_kernel(int n, double sigma) {
  std::vector<float> k(n);
  double sigmaX = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
  double scale2X = -0.5 / (sigmaX * sigmaX);
  double sum = 0;
  for (int i = 0; i < n; i++) {
    double x = i - (n - 1) * 0.5;
    double t = ::exp(scale2X * x * x);
    k[i] = (float)t;
    sum += k[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < n; i++) k[i] = (float)(k[i] * sum);
  return k;
}

inline void GaussianBlur(const Mat &src, Mat &dst, Size ksize, double sx, double sy, int border) {
  assert(border == BORDER_REPLICATE && src.tp == CV_32F && ksize.width % 2 == 1 && ksize.height % 2 == 1);
  const int rows = src.rows, cols = src.cols, kx = cols == 1 ? 1 : ksize.width, ky = rows == 1 ? 1 : ksize.height;
  const std::vector<float> KX = gaussian_kernel(kx, sx), KY = gaussian_kernel(ky, sy);
  const int rx = kx / 2, ry = ky / 2;
  Mat tmp(rows, cols, CV_32F), out(rows, cols, CV_32F);
  for (int r = 0; r < rows; r++) {
    const float *s = src.ptr<float>(r);
    float *d = tmp.ptr<float>(r);
    for (int c = 0; c < cols; c++) {
      float v;
      if (kx <= 5) {
        v = s[c] * KX[rx];
        for (int j = 1; j <= rx; j++) v = v + (s[border_replicate(c - j, cols)] + s[border_replicate(c + j, cols)]) * KX[rx + j];
      } else {
        v = 0.f;
        for (int j = 0; j < kx; j++) v = v + s[border_replicate(c + j - rx, cols)] * KX[j];
      }
      d[c] = v;
    }
  }
  for (int r = 0; r < rows; r++) {
    float *d = out.ptr<float>(r);
    const float *S0 = tmp.ptr<float>(r);
    for (int c = 0; c < cols; c++) d[c] = KY[ry] * S0[c] + 0.f;
    for (int j = 1; j <= ry; j++) {
      const float *Sa = tmp.ptr<float>(border_replicate(r + j, rows)), *Sb = tmp.ptr<float>(border_replicate(r - j, rows));
      for (int c = 0; c < cols; c++) d[c] = d[c] + KY[ry + j] * (Sa[c] + Sb[c]);
    }
  }
  out.copyTo(dst);
}

// kx filters along a row, ky along a column
inline void sepFilter2D(const Mat &src, Mat &dst, int ddepth, const Mat &kx, const Mat &ky) {
  assert(ddepth == CV_32F && src.tp == CV_32F && kx.tp == CV_32F && ky.tp == CV_32F);
  const int rows = src.rows, cols = src.cols, nx = kx.rows * kx.cols, ny = ky.rows * ky.cols, rx = nx / 2, ry = ny / 2;
  const float *KX = kx.ptr<float>(0), *KY = ky.ptr<float>(0);
  Mat tmp(rows, cols, CV_32F), out(rows, cols, CV_32F);
  for (int r = 0; r < rows; r++) {
    const float *s = src.ptr<float>(r);
    float *d = tmp.ptr<float>(r);
    for (int c = 0; c < cols; c++) {
      float v = s[border_reflect101(c - rx, cols)] * KX[0];
      for (int j = 1; j < nx; j++) v = v + s[border_reflect101(c + j - rx, cols)] * KX[j];
      d[c] = v;
    }
  }
  for (int r = 0; r < rows; r++) {
    float *d = out.ptr<float>(r);
    for (int c = 0; c < cols; c++) {
      float v = tmp.ptr<float>(border_reflect101(r - ry, rows))[c] * KY[0];
      for (int j = 1; j < ny; j++) v = v + tmp.ptr<float>(border_reflect101(r + j - ry, rows))[c] * KY[j];
      d[c] = v;
    }
  }
  out.copyTo(dst);
}

// ksize <= 0: the 3-tap Scharr pair, [-1, 0, 1] for order 1 and [3, 10, 3] (over 32 when normalised) for order 0
inline void getDerivKernels(OutputArray kx, OutputArray ky, int dx, int dy, int ksize, bool normalize = false, int ktype = CV_32F) {
  assert(ksize <= 0 && ktype == CV_32F && dx >= 0 && dy >= 0 && dx + dy == 1);
  for (int k = 0; k < 2; k++) {
    OutputArray out = k == 0 ? kx : ky;
    const int order = k == 0 ? dx : dy;
    out.create(3, 1, CV_32F);
    float *p = out.getMat().ptr<float>(0);
    const double scale = !normalize || order == 1 ? 1. : 1. / 32;
    const int v[2][3] = {{3, 10, 3}, {-1, 0, 1}};
    for (int t = 0; t < 3; t++) p[t] = (float)(v[order][t] * scale);
  }
}

inline void Scharr(const Mat &src, Mat &dst, int ddepth, int dx, int dy, double scale = 1, double delta = 0, int border = BORDER_DEFAULT) {
  assert(scale == 1 && delta == 0 && border == BORDER_DEFAULT);
  Mat kx, ky;
  getDerivKernels(kx, ky, dx, dy, -1, false, CV_32F);
  sepFilter2D(src, dst, ddepth, kx, ky);
}

struct AreaTab { int si; float alpha; };
// the INTER_AREA table of one axis: per destination index the source cells it covers and their weights
inline std::vector<std::vector<AreaTab> > area_table(int ssize, int dsize) {
  std::vector<std::vector<AreaTab> > tab(dsize);
  const double scale = ssize / (double)dsize;
  for (int d = 0; d < dsize; d++) {
    const double fs1 = d * scale, fs2 = fs1 + scale, cell = std::min(scale, ssize - fs1);
    int s1 = (int)::ceil(fs1), s2 = (int)::floor(fs2);
    s2 = std::min(s2, ssize - 1);
    s1 = std::min(s1, s2);
    if (s1 - fs1 > 1e-3) { AreaTab t = {s1 - 1, (float)((s1 - fs1) / cell)}; tab[d].push_back(t); }
    for (int s = s1; s < s2; s++) { AreaTab t = {s, (float)(1.0 / cell)}; tab[d].push_back(t); }
    if (fs2 - s2 > 1e-3) { AreaTab t = {s2, (float)(std::min(std::min(fs2 - s2, 1.), cell) / cell)}; tab[d].push_back(t); }
  }
  return tab;
}

inline void resize(const Mat &src, Mat &dst, Size dsize, double fx, double fy, int interp) {
  assert(interp == INTER_AREA && fx == 0 && fy == 0 && src.tp == CV_32F);
  const int sr = src.rows, sc = src.cols, dr = dsize.height, dc = dsize.width;
  Mat out(dr, dc, CV_32F);
  if (sr == 2 * dr && sc == 2 * dc) {
    for (int r = 0; r < dr; r++) {
      const float *a = src.ptr<float>(2 * r), *b = src.ptr<float>(2 * r + 1);
      float *d = out.ptr<float>(r);
      for (int c = 0; c < dc; c++) d[c] = (((a[2 * c] + a[2 * c + 1]) + b[2 * c]) + b[2 * c + 1]) * 0.25f;
    }
  } else {
    const std::vector<std::vector<AreaTab> > xt = area_table(sc, dc), yt = area_table(sr, dr);
    std::vector<float> buf(dc);
    for (int r = 0; r < dr; r++) {
      float *sum = out.ptr<float>(r);
      for (size_t k = 0; k < yt[r].size(); k++) {
        const float *S = src.ptr<float>(yt[r][k].si);
        const float beta = yt[r][k].alpha;
        for (int c = 0; c < dc; c++) {
          float v = 0.f;
          for (size_t j = 0; j < xt[c].size(); j++) v += S[xt[c][j].si] * xt[c][j].alpha;
          buf[c] = v;
        }
        if (k == 0) for (int c = 0; c < dc; c++) sum[c] = beta * buf[c];
        else for (int c = 0; c < dc; c++) sum[c] += beta * buf[c];
      }
    }
  }
  out.copyTo(dst);
}

inline bool solve(const Mat &A, const Mat &b, Mat &dst, int flags) {
  assert(flags == DECOMP_LU && A.rows == 2 && A.cols == 2 && b.rows == 2 && b.cols == 1 && dst.rows == 2 && dst.cols == 1);
  const float *a = A.ptr<float>(0), *bb = b.ptr<float>(0);
  float *x = dst.ptr<float>(0);
  double d = (double)a[0] * a[3] - (double)a[1] * a[2];
  if (d != 0.) {
    d = 1. / d;
    const double t = ((double)bb[0] * a[3] - (double)bb[1] * a[1]) * d;
    x[1] = (float)(((double)bb[1] * a[0] - (double)bb[0] * a[2]) * d);
    x[0] = (float)t;
    return true;
  }
  return false;
}

}  // namespace cv
