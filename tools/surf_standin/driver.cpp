// The driver of tools/make_surf_fixture.py: C entries around the reference's OpenSURF descriptor, compiled together with its
// opensurf/surf.cpp and opensurf/integral.cpp against the stand-in opencv/cv.h of this directory.
//   * getGray (opensurf/utils.cpp:62-82, not compiled: it needs highgui) is restated for the one-channel f32 image the functor
//     hands it: a clone, then cvConvertScale(., ., 1.0 / 255.0, 0), which OpenCV 2.4 evaluates per pixel in f32 as
//     p * (float)(1.0 / 255.0) + 0.0f (restated from knowledge of OpenCV 2.4, not from its source);
//   * SURFDescriptor (descriptors/surfdescriptor.hpp:13-37) is restated: one upright point at x = y = patchSize / 2.0f of scale
//     (float)(patchSize / mrSize), Integral of the patch, getDescriptors(true);
//   * surf_tables restates the coordinate and weight expressions of getDescriptor(true) and the two gaussian overloads behind the
//     same headers, so that an unqualified exp resolves here as it does in surf.cpp.  The descriptors pin them: the model of
//     tests/surf_model.py reproduces every recorded descriptor from these tables bit for bit.
#include <vector>
#include "utils.h"
#include "surf.h"

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

static const float kPi = 3.14159f;
static float gauss_i(int x, int y, float sig) { return (1.0f / (2.0f * kPi * sig * sig)) * exp(-(x * x + y * y) / (2.0f * sig * sig)); }
static float gauss_f(float x, float y, float sig) { return 1.0f / (2.0f * kPi * sig * sig) * exp(-(x * x + y * y) / (2.0f * sig * sig)); }

extern "C" {

// desc[64]; integral[patchSize * patchSize] (optional): the integral image the descriptor was read from
void surf_ref(const float *patch, int patchSize, double mrSize, float *desc, float *integral) {
  std::vector<float> copy(patch, patch + (size_t)patchSize * patchSize);
  IplImage hdr;
  hdr.nChannels = 1; hdr.depth = IPL_DEPTH_32F; hdr.width = patchSize; hdr.height = patchSize;
  hdr.widthStep = patchSize * 4; hdr.imageData = (char *)copy.data();
  IpVec ipts;
  Ipoint pt;
  pt.x = (float)patchSize / 2.0f;
  pt.y = (float)patchSize / 2.0f;
  pt.orientation = 0.0f;
  pt.scale = float(patchSize) / mrSize;
  ipts.push_back(pt);
  IplImage *int_img = Integral(&hdr);
  Surf des(int_img, ipts);
  des.getDescriptors(true);
  for (int i = 0; i < 64; i++) desc[i] = ipts[0].descriptor[i];
  if (integral)
    for (int r = 0; r < patchSize; r++)
      memcpy(integral + (size_t)r * patchSize, int_img->imageData + (size_t)r * int_img->widthStep, (size_t)patchSize * 4);
  cvReleaseImage(&int_img);
}

// sample_x[24] (k = -12 .. 11), sample_y[24] (l = -12 .. 11), w1[16][81], w2[16], the Haar size
void surf_tables(int patchSize, double mrSize, int *sample_x24, int *sample_y24, float *w1, float *w2, int *haar_size) {
  const float scale = float(patchSize) / mrSize;
  const int x = fRound((float)patchSize / 2.0f), y = fRound((float)patchSize / 2.0f);
  const float co = 1, si = 0;
  float cx = -0.5f, cy = 0.f;
  int q = 0;
  for (int i = -12; i < 8; i += 5) {
    cx += 1.f;
    cy = -0.5f;
    for (int j = -12; j < 8; j += 5, q++) {
      cy += 1.f;
      const int ix = i + 5, jx = j + 5;
      const int xs = fRound(x + (-jx * scale * si + ix * scale * co));
      const int ys = fRound(y + (jx * scale * co + ix * scale * si));
      int t = 0;
      for (int k = i; k < i + 9; ++k)
        for (int l = j; l < j + 9; ++l, ++t) {
          const int sample_x = fRound(x + (-l * scale * si + k * scale * co));
          const int sample_y = fRound(y + (l * scale * co + k * scale * si));
          sample_x24[k + 12] = sample_x;
          sample_y24[l + 12] = sample_y;
          w1[q * 81 + t] = gauss_i(xs - sample_x, ys - sample_y, 2.5f * scale);
        }
      w2[q] = gauss_f(cx - 2.0f, cy - 2.0f, 1.5f);
    }
  }
  *haar_size = 2 * fRound(scale);
}

}
