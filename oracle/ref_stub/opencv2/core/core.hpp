/* TEST INFRASTRUCTURE ONLY.  This stands in for OpenCV's <opencv2/core/core.hpp> only so that the reference's MSER translation
 * units (detectors/mser/extrema, compiled in place by oracle/Makefile) parse: they name cv::Mat in declarations and in the dead
 * doOnWLD branch of DetectMSERs.  The MSER path that runs reads Mat::rows, Mat::cols and Mat::data and nothing else; no cv::
 * operation that it executes lives here.  <string> is here because the reference's structures.hpp uses std::string without it. */
#ifndef MODSX_REF_STUB_OPENCV_CORE_HPP
#define MODSX_REF_STUB_OPENCV_CORE_HPP
#include <string>

namespace cv {
struct Mat {
  int rows = 0, cols = 0;
  unsigned char *data = nullptr;
};
/* parsed by the doOnWLD branch (extrema.cpp:317), never run: the shim leaves doOnWLD = 0 */
inline Mat operator+(const Mat &m, double) { return m; }
inline Mat operator*(const Mat &m, double) { return m; }
}  // namespace cv
#endif
