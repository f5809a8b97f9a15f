// A stand-in for <opencv/cv.h>, just wide enough for tools/make_surf_fixture.py to compile the reference's opensurf/surf.cpp and
// opensurf/integral.cpp without OpenCV: a single-channel image header that owns its pixels, with rows of 4-byte aligned step as
// cvCreateImage lays them out.  Not OpenCV and not for anything else.
#pragma once
#include <math.h>   // OpenCV's C headers bring in the C header (the reference's ipoint.h includes it too)
#include <stdlib.h>
#include <string.h>

#define IPL_DEPTH_8U 8
#define IPL_DEPTH_32F 32

struct CvPoint { int x, y; };
struct CvSize { int width, height; };

struct IplImage {
  int nChannels, depth, width, height, widthStep;
  char *imageData;
};

inline CvSize cvGetSize(const IplImage *img) {
  CvSize s = {img->width, img->height};
  return s;
}
inline IplImage *cvCreateImage(CvSize size, int depth, int channels) {
  IplImage *img = (IplImage *)malloc(sizeof(IplImage));
  img->nChannels = channels; img->depth = depth; img->width = size.width; img->height = size.height;
  img->widthStep = (size.width * channels * (depth / 8) + 3) & ~3;
  img->imageData = (char *)calloc((size_t)img->widthStep * size.height, 1);
  return img;
}
inline void cvReleaseImage(IplImage **img) {
  if (img && *img) { free((*img)->imageData); free(*img); *img = 0; }
}
