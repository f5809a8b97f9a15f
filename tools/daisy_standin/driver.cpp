// The driver of tools/make_daisy_fixture.py: what descriptors/daisydescriptor.hpp does with one patch, without OpenCV, on top of
// the reference's libdaisy compiled as it is.  Nothing here is part of the library.
//   daisy_ref     bytes = rint-and-saturate of the f32 patch (cv::Mat::convertTo(CV_8U)), then set_image, set_parameters, the
//                 caller's workspace, initialize_single_descriptor_mode, set_normalization and get_descriptor(side / 2, side / 2, 0)
//                 on a zero-filled row.  cubes (may be null): layer `layer` of every cube, read back from the workspace, where
//                 compute_histograms leaves cube c pixel-major at slot c.
//   daisy_grad    the blurred image, dx and dy of layered_gradient, through the same public kutility calls.
//   daisy_consts  the oriented grid of orientation 0 (y, x pairs), g_selected_cubes and a gaussian_1d of a given length.
#include <math.h>
#include <string.h>
#include <vector>
#include "daisy/daisy.h"

static void to_bytes(const float *patch, int n, unsigned char *b) {
  for (int i = 0; i < n; i++) {
    const double r = nearbyint((double)patch[i]);      // round half to even, the default rounding mode
    b[i] = (unsigned char)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
  }
}

extern "C" int daisy_ref(const float *patch, int side, int rad, int radq, int thq, int histq, int nrm, float *desc, int layer,
                         float *cubes) {
  std::vector<unsigned char> im(side * side);
  to_bytes(patch, side * side, im.data());
  daisy *d = new daisy();
  d->set_image(im.data(), side, side);
  d->verbose(0);
  d->set_parameters(rad, radq, thq, histq);
  const int ws = d->compute_workspace_memory();
  std::vector<float> work(ws);
  d->set_workspace_memory(work.data(), ws);
  d->initialize_single_descriptor_mode();
  d->set_normalization(nrm);
  const int dim = d->descriptor_size();
  memset(desc, 0, sizeof(float) * dim);
  d->get_descriptor((double)(side / 2), (double)(side / 2), 0, desc);
  if (cubes)
    for (int c = 0; c < radq; c++)
      for (int p = 0; p < side * side; p++) cubes[c * side * side + p] = work[(size_t)c * side * side * histq + (size_t)p * histq + layer];
  d->release_auxilary();
  delete d;
  return dim;
}

extern "C" void daisy_grad(const float *patch, int side, float *blurred, float *dx, float *dy) {
  const int n = side * side;
  std::vector<unsigned char> im(n);
  to_bytes(patch, n, im.data());
  float *f = kutility::type_cast<float, unsigned char>(im.data(), n);
  kutility::divide(f, n, (float)255.0);
  float kernel[5];
  kutility::gaussian_1d(kernel, 5, 0.5, 0);
  kutility::convolve_sym(f, side, side, kernel, 5);
  kutility::gradient(f, side, side, dy, dx);
  memcpy(blurred, f, sizeof(float) * n);
  kutility::deallocate(f);
}

extern "C" void daisy_consts(int side, int rad, int radq, int thq, int histq, double *grid_yx, int *selected, int fsz, float sigma,
                             float *taps) {
  if (grid_yx) {
    std::vector<unsigned char> im(side * side, 0);
    daisy *d = new daisy();
    d->set_image(im.data(), side, side);
    d->verbose(0);
    d->set_parameters(rad, radq, thq, histq);
    memcpy(grid_yx, d->get_grid(0), sizeof(double) * 2 * (radq * thq + 1));
    for (int r = 0; r < radq; r++) selected[r] = g_selected_cubes[r];
    d->release_auxilary();
    delete d;
  }
  if (taps) kutility::gaussian_1d(taps, fsz, sigma, 0);
}
