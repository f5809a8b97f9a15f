// The driver of tools/make_surfdet_fixture.py: one C entry around the reference's OpenSURF detector, compiled together with its
// opensurf/fasthessian.cpp and opensurf/integral.cpp against the stand-in opencv/cv.h of this directory.
//   * getGray (opensurf/utils.cpp:62-82, not compiled: it needs highgui) is restated for a one-channel f32 image as in
//     tools/surf_standin/driver.cpp: p * (float)(1.0 / 255.0) + 0.0f per pixel;
//   * the SURF branch of imagerepresentation.cpp:1046-1076 is restated: Integral of the image, FastHessian(int_img, ipts, octaves,
//     intervals, init_sample, thres), getIpoints();
//   * the response planes and the raw extremum list are read from the object after getIpoints(): this file alone sees the class
//     with its private members opened (the layout is unchanged), walks responseMap and asks isExtremum in getIpoints' loop order.
#include <vector>
#include "utils.h"
#include "integral.h"
#include "responselayer.h"
#define private public
#include "fasthessian.h"
#undef private

IplImage *getGray(const IplImage *img) {
  IplImage *gray32 = cvCreateImage(cvGetSize(img), IPL_DEPTH_32F, 1);
  const float scale = (float)(1.0 / 255.0), shift = 0.0f;
  for (int r = 0; r < img->height; r++) {
    const float *s = (const float *)(img->imageData + (size_t)r * img->widthStep);
    float *d = (float *)(gray32->imageData + (size_t)r * gray32->widthStep);
    for (int c = 0; c < img->width; c++) d[c] = s[c] * scale + shift;
  }
  return gray32;
}

extern "C" {

// integral [rows][cols]; layers [12][4] (width, height, step, filter); resp / lap: the planes one after the other (capPlane
// values in all); ipts [capPts][3] (x, y, scale) with iptsLap [capPts]; ext [capPts][4] (o, i, r, c).
// counts [4] = layers, plane values, points, extrema.  Returns 0, or -1 when a buffer is too small (counts are still filled).
int surfdet_ref(const float *pixels, int rows, int cols, int octaves, int intervals, int init_sample, float thres, float *integral,
                int *layers, float *resp, unsigned char *lap, long capPlane, float *ipts, int *iptsLap, int *ext, int capPts,
                long *counts) {
  std::vector<float> copy(pixels, pixels + (size_t)rows * cols);
  IplImage hdr;
  hdr.nChannels = 1; hdr.depth = IPL_DEPTH_32F; hdr.width = cols; hdr.height = rows;
  hdr.widthStep = cols * 4; hdr.imageData = (char *)copy.data();
  IplImage *int_img = Integral(&hdr);
  for (int r = 0; r < rows; r++) memcpy(integral + (size_t)r * cols, int_img->imageData + (size_t)r * int_img->widthStep, (size_t)cols * 4);
  IpVec pts;
  FastHessian fh(int_img, pts, octaves, intervals, init_sample, thres);
  fh.getIpoints();
  int rc = 0;
  long used = 0;
  counts[0] = (long)fh.responseMap.size();
  for (size_t k = 0; k < fh.responseMap.size(); k++) {
    const ResponseLayer *L = fh.responseMap[k];
    layers[4 * k] = L->width; layers[4 * k + 1] = L->height; layers[4 * k + 2] = L->step; layers[4 * k + 3] = L->filter;
    const long n = (long)L->width * L->height;
    if (used + n <= capPlane) { memcpy(resp + used, L->responses, n * 4); memcpy(lap + used, L->laplacian, n); } else rc = -1;
    used += n;
  }
  counts[1] = used;
  counts[2] = (long)pts.size();
  for (size_t k = 0; k < pts.size() && (int)k < capPts; k++) {
    ipts[3 * k] = pts[k].x; ipts[3 * k + 1] = pts[k].y; ipts[3 * k + 2] = pts[k].scale; iptsLap[k] = pts[k].laplacian;
  }
  static const int filter_map[OCTAVES][INTERVALS] = {{0, 1, 2, 3}, {1, 3, 4, 5}, {3, 5, 6, 7}, {5, 7, 8, 9}, {7, 9, 10, 11}};
  long ne = 0;
  for (int o = 0; o < fh.octaves; ++o)
    for (int i = 0; i <= 1; ++i) {
      ResponseLayer *b = fh.responseMap.at(filter_map[o][i]), *m = fh.responseMap.at(filter_map[o][i + 1]),
                    *t = fh.responseMap.at(filter_map[o][i + 2]);
      for (int r = 0; r < t->height; ++r)
        for (int c = 0; c < t->width; ++c)
          if (fh.isExtremum(r, c, t, m, b)) {
            if (ne < capPts) { ext[4 * ne] = o; ext[4 * ne + 1] = i; ext[4 * ne + 2] = r; ext[4 * ne + 3] = c; }
            ne++;
          }
    }
  counts[3] = ne;
  if ((long)pts.size() > capPts || ne > capPts) rc = -1;
  cvReleaseImage(&int_img);
  return rc;
}

}
