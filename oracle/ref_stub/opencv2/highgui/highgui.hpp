/* TEST INFRASTRUCTURE ONLY.  This stands in for OpenCV's <opencv2/highgui/highgui.hpp> only so that the reference's MSER translation
 * units parse: the dead doOnWLD branch of DetectMSERs (extrema.cpp:319) names imwrite.  Nobody calls it -- the shim leaves
 * doOnWLD = 0 -- and oracle/ref_mser_shim.cpp defines it as abort(). */
#ifndef MODSX_REF_STUB_OPENCV_HIGHGUI_HPP
#define MODSX_REF_STUB_OPENCV_HIGHGUI_HPP
#include <opencv2/core/core.hpp>

namespace cv {
bool imwrite(const std::string &name, const Mat &img);
}
#endif
