// A stand-in for <opencv/cv.h>, just wide enough for tools/make_surfdet_fixture.py to compile the reference's
// opensurf/fasthessian.cpp and opensurf/integral.cpp without OpenCV: a single-channel image header that owns its pixels (rows of
// 4-byte aligned step, as cvCreateImage lays them out) and the few CvMat calls of FastHessian::interpolateStep on f64 matrices.
// cvInvert is NOT OpenCV's SVD inverse: it is the library's specification of that step, the closed-form adjugate inverse in f64
// with the order of operations of mods_amd/csrc/kernels_surfdet.hip (sd_inv3) and tests/surfdet_model.py (inv3); all zeros where
// the determinant is 0 or not finite.  cvGEMM covers the one form the reference calls: dst = alpha * A * B, in row order, each
// dot product added from the left.  Not OpenCV and not for anything else.
#pragma once
#include <assert.h>
#include <math.h>   // OpenCV's C headers bring in the C headers (the reference's sources rely on it)
#include <stdlib.h>
#include <string.h>

#define IPL_DEPTH_8U 8
#define IPL_DEPTH_32F 32
#define CV_64FC1 6
#define CV_SVD 1
#define CV_AUTOSTEP 0x7fffffff

struct CvPoint { int x, y; };
struct CvSize { int width, height; };

struct IplImage {
  int nChannels, depth, width, height, widthStep;
  char *imageData;
};

inline CvSize cvGetSize(const IplImage *img) {
  CvSize s = {img->width, img->height};
  return s;
}
inline IplImage *cvCreateImage(CvSize size, int depth, int channels) {
  IplImage *img = (IplImage *)malloc(sizeof(IplImage));
  img->nChannels = channels; img->depth = depth; img->width = size.width; img->height = size.height;
  img->widthStep = (size.width * channels * (depth / 8) + 3) & ~3;
  img->imageData = (char *)calloc((size_t)img->widthStep * size.height, 1);
  return img;
}
inline void cvReleaseImage(IplImage **img) {
  if (img && *img) { free((*img)->imageData); free(*img); *img = 0; }
}

struct CvMat {
  int rows, cols, owns;
  double *d;
};
inline CvMat *cvCreateMat(int rows, int cols, int type) {
  assert(type == CV_64FC1);
  CvMat *m = (CvMat *)malloc(sizeof(CvMat));
  m->rows = rows; m->cols = cols; m->owns = 1;
  m->d = (double *)calloc((size_t)rows * cols, sizeof(double));
  return m;
}
inline void cvReleaseMat(CvMat **m) {
  if (m && *m) { if ((*m)->owns) free((*m)->d); free(*m); *m = 0; }
}
inline CvMat *cvInitMatHeader(CvMat *m, int rows, int cols, int type, void *data, int step) {
  assert(type == CV_64FC1 && step == CV_AUTOSTEP);
  m->rows = rows; m->cols = cols; m->owns = 0; m->d = (double *)data;
  return m;
}
inline void cvmSet(CvMat *m, int row, int col, double v) { m->d[row * m->cols + col] = v; }
inline double cvInvert(const CvMat *src, CvMat *dst, int method) {
  assert(method == CV_SVD && src->rows == 3 && src->cols == 3 && dst->rows == 3 && dst->cols == 3);
  const double *S = src->d;
  double *t = dst->d;
  double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
  if (d == 0. || !(fabs(d) <= 1.7976931348623157e308)) { for (int i = 0; i < 9; i++) t[i] = 0; return 0; }
  d = 1. / d;
  t[0] = (S[4] * S[8] - S[5] * S[7]) * d; t[1] = (S[2] * S[7] - S[1] * S[8]) * d; t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
  t[3] = (S[5] * S[6] - S[3] * S[8]) * d; t[4] = (S[0] * S[8] - S[2] * S[6]) * d; t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
  t[6] = (S[3] * S[7] - S[4] * S[6]) * d; t[7] = (S[1] * S[6] - S[0] * S[7]) * d; t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
  return 1;
}
inline void cvGEMM(const CvMat *A, const CvMat *B, double alpha, const CvMat *C, double beta, CvMat *dst, int flags) {
  assert(!C && beta == 0 && flags == 0 && A->rows == 3 && A->cols == 3 && B->rows == 3 && B->cols == 1);
  for (int i = 0; i < 3; i++)
    dst->d[i] = alpha * (A->d[3 * i] * B->d[0] + A->d[3 * i + 1] * B->d[1] + A->d[3 * i + 2] * B->d[2]);
}
