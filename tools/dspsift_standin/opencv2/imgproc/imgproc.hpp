// A stand-in for <opencv2/imgproc/imgproc.hpp> (see ../core/core.hpp).  The fixture's driver hands normalised patches to the
// descriptor and never blurs: a call of GaussianBlur means the tool is being used for something it cannot do.
#pragma once
#include "../core/core.hpp"

namespace cv {

inline void GaussianBlur(const Mat &, Mat &, Size, double, double, int = BORDER_DEFAULT) {
  std::cerr << "dspsift stand-in: GaussianBlur is not available" << std::endl;
  abort();
}

}  // namespace cv
