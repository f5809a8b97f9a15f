/* TEST INFRASTRUCTURE ONLY.  C entry point of oracle/_ref/libmser_ref.so: the reference's own MSER detector, compiled in place
 * from $(REF)/detectors/mser (oracle/Makefile), called the way DetectAffineRegions instantiates it (imagerepresentation.cpp:1037,
 * 2611): the 5-argument DetectMSERs(input, out, params, ScalePyramid &, tilt, zoom) of extrema.cpp:284-473.
 *
 * The pixels go in as f32 through Mat::data, so the reference's own `(unsigned char)*in_ptr` (extrema.cpp:401-403) runs.  The nine
 * fields DetectMSERs sets are copied out; octave_number and pyramid_scale are never written by the reference and are not read.
 * The reference keeps its state in file-level statics: the caller serialises (oracle/pyoracle.py holds one lock). */
#include <cstdlib>
#include <vector>

#include "extrema.h"
#include <opencv2/highgui/highgui.hpp>

/* Only the 4-argument overload of DetectMSERs calls this (extrema.cpp:243); its definition lives in helpers.cpp, which needs OpenCV. */
void rectifyAffineTransformationUpIsUp(double &, double &, double &, double &) { abort(); }
/* named by the doOnWLD branch only, which the shim never enables */
bool cv::imwrite(const std::string &, const cv::Mat &) { abort(); }

extern "C" int refmser_detect(const float *img, int rows, int cols, int relative, int min_size, double max_area, double min_margin,
                              int mode, double rel_threshold, int reg_number, double rel_reg_number, double tilt, double zoom,
                              double *out9, int cap) {
  extrema::ExtremaParams p;
  p.relative = relative != 0;
  p.min_size = min_size;
  p.max_area = max_area;
  p.min_margin = min_margin;
  p.doOnWLD = 0;
  p.doOnNormal = 1;
  p.DetectorMode = (detection_mode_t)mode;
  p.rel_threshold = (float)rel_threshold;
  p.reg_number = reg_number;
  p.rel_reg_number = (float)rel_reg_number;
  cv::Mat m;
  m.rows = rows;
  m.cols = cols;
  m.data = (unsigned char *)img;
  ScalePyramid pyr;
  std::vector<AffineKeypoint> keys;
  const int n = DetectMSERs(m, keys, p, pyr, tilt, zoom);
  for (int i = 0; i < n && i < cap; i++) {
    const AffineKeypoint &k = keys[i];
    double *o = out9 + 9 * (size_t)i;
    o[0] = k.x; o[1] = k.y; o[2] = k.a11; o[3] = k.a12; o[4] = k.a21; o[5] = k.a22; o[6] = k.s; o[7] = k.response;
    o[8] = (double)k.sub_type;
  }
  return n;
}
