// The OpenCV arithmetic of cv_arith.h, forwarded to the oracle's [OCV] primitives -- TEST INFRASTRUCTURE, OUR code.
// The log and every scratch copy use malloc directly, so that nothing here enters the allocation stream of the reference's
// own containers (orbextractor_shim.cc orders that stream).
#include "cv_arith.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "../orb_oracle.h"

namespace
{
const int kEdge = 19;   // EDGE_THRESHOLD, ORBextractor.cc:74: the frame ComputePyramid keeps around every level

[[noreturn]] void unsupported(const char* what)
{
    fprintf(stderr, "[cv_arith] %s: not provided (only the calls ORBextractor.cc makes are)\n", what);
    abort();
}

// BORDER_REFLECT_101 (cv::borderInterpolate): -k -> k, n-1+k -> n-1-k; a single pixel reflects onto itself
int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// a private copy of a CV_8U plane (the reference hands the same Mat in as source and destination)
uint8_t* copy_plane(const cv::Mat& m)
{
    uint8_t* buf = (uint8_t*)malloc((size_t)m.rows * m.cols + 1);
    for (int y = 0; y < m.rows; y++) memcpy(buf + (size_t)y * m.cols, m.data + (size_t)y * m.step, (size_t)m.cols);
    return buf;
}

cv_fast_call* g_calls = NULL;
int g_ncalls = 0, g_calls_cap = 0;
int* g_corners = NULL;
int g_ncorners = 0, g_corners_cap = 0;   // in triplets
}  // namespace

void cv_fast_log_clear() { g_ncalls = g_ncorners = 0; }
int cv_fast_log_size() { return g_ncalls; }
const cv_fast_call* cv_fast_log_calls() { return g_calls; }
const int* cv_fast_log_corners() { return g_corners; }
int cv_fast_log_ncorners() { return g_ncorners; }

namespace cv
{
float fastAtan2(float y, float x) { return orc_fast_atan2(y, x); }

// FAST_t<16> with non-maximum suppression (the oracle's orc_fast9_nms): the output is cleared, then KeyPoint(x, y, 7, -1, score)
// in the order the scan finds them, coordinates relative to the ROI.  Only the ROI is read.
void FAST(InputArray image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmaxSuppression)
{
    if (!nonmaxSuppression) unsupported("FAST without non-maximum suppression");
    const Mat m = image.getMat();
    if (m.type() != CV_8UC1) unsupported("FAST on a non-CV_8UC1 image");
    keypoints.clear();
    const int cap = m.rows * m.cols;
    if (g_ncorners + cap > g_corners_cap) {
        g_corners_cap = 2 * (g_ncorners + cap) + 1024;
        g_corners = (int*)realloc(g_corners, sizeof(int) * 3 * (size_t)g_corners_cap);
    }
    int* xys = g_corners + 3 * (size_t)g_ncorners;
    const int n = m.empty() ? 0 : orc_fast9_nms(m.data, m.cols, m.rows, (int)m.step, threshold, xys, cap);
    for (int k = 0; k < n; k++) keypoints.push_back(KeyPoint((float)xys[3 * k], (float)xys[3 * k + 1], 7.f, -1, (float)xys[3 * k + 2]));
    if (g_ncalls == g_calls_cap) {
        g_calls_cap = g_calls_cap ? 2 * g_calls_cap : 256;
        g_calls = (cv_fast_call*)realloc(g_calls, sizeof(cv_fast_call) * (size_t)g_calls_cap);
    }
    Size whole;
    Point ofs;
    m.locateROI(whole, ofs);
    cv_fast_call& c = g_calls[g_ncalls++];
    c.level_w = whole.width - 2 * kEdge;
    c.level_h = whole.height - 2 * kEdge;
    c.x = ofs.x - kEdge;
    c.y = ofs.y - kEdge;
    c.w = m.cols;
    c.h = m.rows;
    c.threshold = threshold;
    c.first = g_ncorners;
    c.count = n;
    g_ncorners += n;
}

// INTER_LINEAR on CV_8UC1 (orc_resize_linear_u8, the [OCV] resize switch): the source ROI only, into dst created at dsize
// (a view of the right size stays a view).  Equal sizes are a copy, as cv::resize short-cuts them.
void resize(InputArray src_, OutputArray dst_, Size dsize, double fx, double fy, int interpolation)
{
    if (interpolation != INTER_LINEAR || fx != 0 || fy != 0) unsupported("resize other than INTER_LINEAR to a given size");
    // a level that rounds to no pixels: cv::resize asserts (a cv::Exception the reference does not catch)
    if (dsize.width <= 0 || dsize.height <= 0) throw std::runtime_error("cv::resize: empty destination size");
    const Mat src = src_.getMat();
    if (src.type() != CV_8UC1 || src.empty()) unsupported("resize of an empty or non-CV_8UC1 image");
    dst_.create(dsize.height, dsize.width, CV_8UC1);
    Mat dst = dst_.getMat();
    if (dsize.width == src.cols && dsize.height == src.rows) {
        uint8_t* buf = copy_plane(src);
        for (int y = 0; y < dst.rows; y++) memcpy(dst.data + (size_t)y * dst.step, buf + (size_t)y * src.cols, (size_t)dst.cols);
        free(buf);
        return;
    }
    orc_resize_linear_u8(src.data, src.cols, src.rows, (int)src.step, dst.data, dst.cols, dst.rows, (int)dst.step);
}

// 7x7, sigma 2, BORDER_REFLECT_101 on a whole (non-ROI) CV_8UC1 image (orc_gaussian_blur7_u8, the [OCV] blur switches)
void GaussianBlur(InputArray src_, OutputArray dst_, Size ksize, double sigmaX, double sigmaY, int borderType)
{
    if (ksize.width != 7 || ksize.height != 7 || sigmaX != 2 || sigmaY != 2 || borderType != BORDER_REFLECT_101)
        unsupported("GaussianBlur other than 7x7, sigma 2, BORDER_REFLECT_101");
    const Mat src = src_.getMat();
    if (src.type() != CV_8UC1 || src.empty()) unsupported("GaussianBlur of an empty or non-CV_8UC1 image");
    if (src.isSubmatrix()) unsupported("GaussianBlur of a ROI without BORDER_ISOLATED");   // OpenCV would read the parent's pixels
    uint8_t* buf = copy_plane(src);
    dst_.create(src.rows, src.cols, CV_8UC1);
    Mat dst = dst_.getMat();
    orc_gaussian_blur7_u8(buf, src.cols, src.rows, src.cols, dst.data, (int)dst.step);
    free(buf);
}

// BORDER_REFLECT_101, with or without BORDER_ISOLATED.  Without it OpenCV takes the border from the parent's pixels where src is a
// ROI; the reference passes a whole image there (ORBextractor.cc:1196), so that case is refused rather than restated.
void copyMakeBorder(InputArray src_, OutputArray dst_, int top, int bottom, int left, int right, int borderType, const Scalar&)
{
    const int isolated = borderType & BORDER_ISOLATED;
    if ((borderType & ~BORDER_ISOLATED) != BORDER_REFLECT_101) unsupported("copyMakeBorder other than BORDER_REFLECT_101");
    const Mat src = src_.getMat();
    if (src.type() != CV_8UC1 || src.empty()) unsupported("copyMakeBorder of an empty or non-CV_8UC1 image");
    if (!isolated && src.isSubmatrix()) unsupported("copyMakeBorder of a ROI without BORDER_ISOLATED");
    uint8_t* buf = copy_plane(src);   // src is the interior of dst at ORBextractor.cc:1191
    dst_.create(src.rows + top + bottom, src.cols + left + right, CV_8UC1);
    Mat dst = dst_.getMat();
    for (int y = 0; y < dst.rows; y++) {
        const uint8_t* S = buf + (size_t)reflect101(y - top, src.rows) * src.cols;
        uint8_t* D = dst.data + (size_t)y * dst.step;
        for (int x = 0; x < dst.cols; x++) D[x] = S[reflect101(x - left, src.cols)];
    }
    free(buf);
}
}  // namespace cv
