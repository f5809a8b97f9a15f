// A stand-in for <opencv2/core/core.hpp>, just wide enough for tools/make_dspsift_fixture.py to compile the reference's
// matching/siftdesc.cpp and detectors/helpers.cpp without OpenCV: a dense single-channel f32 matrix that owns its storage or
// wraps the caller's, shared between copies.  Not OpenCV and not for anything else.
#pragma once
#include <math.h>   // OpenCV's core headers bring in the C header, and the reference leans on it (M_PI, ::sqrt, fabs)
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#define CV_32F 5
#define CV_32FC1 5
#ifndef MAX
#define MAX(a, b) ((a) < (b) ? (b) : (a))
#endif
#ifndef MIN
#define MIN(a, b) ((a) > (b) ? (b) : (a))
#endif

namespace cv {

struct Size {
  int width, height;
  Size(int w = 0, int h = 0) : width(w), height(h) {}
};

enum { BORDER_REPLICATE = 1, BORDER_DEFAULT = 4 };

class Mat {
 public:
  int rows = 0, cols = 0;
  size_t step = 0;   // bytes per row
  unsigned char *data = nullptr;
  Mat() {}
  Mat(int r, int c, int t) : rows(r), cols(c), step((size_t)c * 4), own_(new std::vector<unsigned char>((size_t)r * c * 4)), type_(t) {
    data = own_->data();
  }
  Mat(int r, int c, int t, void *p) : rows(r), cols(c), step((size_t)c * 4), data((unsigned char *)p), type_(t) {}
  int type() const { return type_; }
  template <typename T> T *ptr(int r = 0) { return (T *)(data + (ptrdiff_t)r * (ptrdiff_t)step); }
  template <typename T> const T *ptr(int r = 0) const { return (const T *)(data + (ptrdiff_t)r * (ptrdiff_t)step); }
  template <typename T> T &at(int r, int c) { return ptr<T>(r)[c]; }
  template <typename T> const T &at(int r, int c) const { return ptr<T>(r)[c]; }
  Mat clone() const {
    Mat m(rows, cols, type_);
    for (int r = 0; r < rows; r++) memcpy(m.ptr<unsigned char>(r), ptr<unsigned char>(r), (size_t)cols * 4);
    return m;
  }

 private:
  std::shared_ptr<std::vector<unsigned char>> own_;
  int type_ = CV_32FC1;
};

}  // namespace cv
