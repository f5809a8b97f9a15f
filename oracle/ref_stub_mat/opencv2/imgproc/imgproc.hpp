/* TEST INFRASTRUCTURE ONLY.  Stands in for OpenCV's <opencv2/imgproc/imgproc.hpp> so that the reference's detectors/helpers.cpp
 * parses: gaussianBlur / gaussianBlurInplace (helpers.cpp:717-731) name GaussianBlur.  Declared only; the pinned entry points never
 * reach it and oracle/ref_hessaff_shim.cpp defines it as "print the name and abort" (see core/core.hpp in this directory). */
#ifndef MODSX_REF_STUB_MAT_OPENCV_IMGPROC_HPP
#define MODSX_REF_STUB_MAT_OPENCV_IMGPROC_HPP
#include <opencv2/core/core.hpp>

namespace cv {
void GaussianBlur(const Mat &src, Mat &dst, Size ksize, double sigmaX, double sigmaY, int borderType);
}
#endif
