// The OpenCV ARITHMETIC that the reference's src/ORBextractor.cc calls, declared as OpenCV 3.4 declares it and forwarded to the
// oracle's [OCV] primitives (oracle/orb_oracle.c) -- TEST INFRASTRUCTURE, OUR code, no OpenCV text.
//
// oracle/Makefile force-includes this header (-include) when it compiles the reference's ORBextractor.cc, unmodified, into
// _ref/libref_orbextractor*.so; the container types come from the stand-in tests/cv_standin/opencv/cv.h.  What the extractor then
// computes is the reference's own logic around five primitives that are the oracle's by construction:
//   cv::FAST(img, kps, th, true)                    -> orc_fast9_nms on the ROI's pointer and stride   (every call is logged)
//   cv::resize(src, dst, sz, 0, 0, INTER_LINEAR)    -> orc_resize_linear_u8 on the source ROI
//   cv::GaussianBlur(7x7, 2, 2, REFLECT_101)        -> orc_gaussian_blur7_u8 (in place allowed: the reference passes src == dst)
//   cv::fastAtan2                                   -> orc_fast_atan2
// plus copyMakeBorder (BORDER_REFLECT_101, with or without BORDER_ISOLATED) and cvFloor / cvCeil, restated here.  Every [OCV]
// switch of the oracle (orc_set_ocv_variant, orc_set_gauss_taps) therefore applies to both sides.
#pragma once
#include <opencv/cv.h>

#include <vector>

// cvFloor / cvCeil as OpenCV 3.4 states them for x86-64 (cvtsd2si / cvtss2si under the default rounding mode, corrected by one where
// the rounded value overshoots); cvRound (round half to even) is the stand-in's own, tests/cv_standin/opencv/cv.h.
static inline int cvFloor(double v) { const int i = (int)lrint(v); return i - (v < (double)i); }
static inline int cvFloor(float v) { const int i = (int)lrintf(v); return i - (v < (float)i); }
static inline int cvFloor(int v) { return v; }
static inline int cvCeil(double v) { const int i = (int)lrint(v); return i + ((double)i < v); }
static inline int cvCeil(float v) { const int i = (int)lrintf(v); return i + ((float)i < v); }
static inline int cvCeil(int v) { return v; }

namespace cv
{
float fastAtan2(float y, float x);
void FAST(InputArray image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmaxSuppression = true);
void resize(InputArray src, OutputArray dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR);
void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY = 0, int borderType = BORDER_DEFAULT);
void copyMakeBorder(InputArray src, OutputArray dst, int top, int bottom, int left, int right, int borderType,
                    const Scalar& value = Scalar());
}  // namespace cv

// The FAST call log (oracle/ref_shim/cv_arith.cc): one record per cv::FAST call since the last cv_fast_log_clear().
struct cv_fast_call {
    int level_w, level_h;   // the level the ROI is a view of (its parent allocation less the 19-px frame)
    int x, y, w, h;         // the ROI within that level
    int threshold;
    int first, count;       // corners [first, first + count) of cv_fast_log_corners(): {x, y, score} relative to the ROI
};
void cv_fast_log_clear();
int cv_fast_log_size();
const cv_fast_call* cv_fast_log_calls();
const int* cv_fast_log_corners();
int cv_fast_log_ncorners();
