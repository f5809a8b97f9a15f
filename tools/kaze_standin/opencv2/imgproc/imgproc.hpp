// part of the stand-in of this directory: everything is in opencv2/opencv.hpp
#pragma once
#include <opencv2/opencv.hpp>
