/* TEST INFRASTRUCTURE ONLY.  Stands in for OpenCV's <opencv2/highgui/highgui.hpp>, which the reference's affinedetectors/affine.h
 * includes and uses nothing of (see core/core.hpp in this directory). */
#ifndef MODSX_REF_STUB_MAT_OPENCV_HIGHGUI_HPP
#define MODSX_REF_STUB_MAT_OPENCV_HIGHGUI_HPP
#include <opencv2/core/core.hpp>
#endif
