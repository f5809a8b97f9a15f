// The driver of tools/make_dspsift_fixture.py: C entries around the reference's SIFTDescriptor, compiled together with its
// matching/siftdesc.cpp and detectors/helpers.cpp against the stand-in headers of this directory.
#include <vector>
#include "matching/siftdesc.h"

static SIFTDescriptorParams params(double maxBinValue, bool doNorm) {
  SIFTDescriptorParams p;          // spatialBins 4, orientationBins 8, useRootSIFT 0, doHalfSIFT 0, magnLess false
  p.PEParam.patchSize = 41;
  p.patchSize = 41;
  p.useRootSIFT = 0;
  p.doNorm = doNorm;
  p.maxBinValue = maxBinValue;
  return p;
}

extern "C" {

// the functor of the DSPSIFT branch (imagerepresentation.cpp:1549-1552) on one normalised 41 x 41 patch: hist[128]
void dsp_raw(const float *patch41, float *hist) {
  SIFTDescriptor d(params(0.2, false));
  std::vector<float> copy(patch41, patch41 + 41 * 41);
  cv::Mat patch(41, 41, CV_32FC1, copy.data());
  std::vector<float> desc;
  d(patch, desc);
  for (int i = 0; i < 128; i++) hist[i] = desc[i];
}

// SIFTnorm(std::vector<float>&) (imagerepresentation.cpp:1593-1597) on one row of 128
void dsp_norm(const float *row, double maxBinValue, float *out) {
  SIFTDescriptor d(params(maxBinValue, true));
  std::vector<float> v(row, row + 128);
  d.SIFTnorm(v);
  for (int i = 0; i < 128; i++) out[i] = v[i];
}

}
