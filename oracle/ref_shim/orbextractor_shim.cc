// C entry points around the REFERENCE's own ORB_SLAM2::ORBextractor -- TEST INFRASTRUCTURE, build container only.
//
// oracle/_ref/libref_orbextractor*.so = this file + cv_arith.cc + the reference's src/ORBextractor.cc compiled UNMODIFIED where it
// lies (oracle/Makefile, target ref), against the container stand-in tests/cv_standin and the arithmetic forwarders of cv_arith.h,
// linked with ../liborb_oracle.so.  Everything the extractor computes outside the five OpenCV primitives -- the constructor tables,
// ComputePyramid's frame and ROIs, the cell grid and its threshold fallback, DistributeOctTree, IC_Angle, computeOrbDescriptor and
// the level layout of operator() -- is the reference's compiled code.
//
// Allocation order.  DistributeOctTree sorts (size, node address) pairs (ORBextractor.cc:684), so equal-sized nodes split in the
// order the allocator placed them.  The oracle fixes that order as "newest first", what a heap whose addresses only grow gives
// (SURVEY.md 0.3).  This file realises exactly that model: while a call runs, the global operator new of this library is a bump
// arena -- one region reserved up front, reset at the start of every call, nothing freed into it ever reused -- so a list node
// created later always has the higher address.  The replacement operators are local to the library (ref_exports.map): only its
// own code (the reference's containers) binds to them.  ref_set_system_allocator(1) sends the calls to malloc / free instead
// (glibc's reuse of freed nodes), for counting how often that changes the result; ref_arena_stats proves which one served the
// reference's list nodes.
#include <sys/mman.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <list>
#include <new>
#include <vector>

#include "../orb_oracle.h"
#include "ORBextractor.h"
#include "cv_arith.h"

#define EXPORT extern "C"

namespace
{
char* g_base = NULL;          // the arena: one reservation, never extended
size_t g_cap = 0, g_used = 0;
bool g_active = false;        // a shim call is running
bool g_system = false;        // ref_set_system_allocator
long long g_stats[5];         // arena allocations, list-node allocations, malloc allocations during calls, arena bytes, arena overflows
const size_t kListNode = sizeof(std::_List_node<ORB_SLAM2::ExtractorNode>);

bool in_arena(const void* p) { return g_base && (const char*)p >= g_base && (const char*)p < g_base + g_cap; }

bool reserve()
{
    if (g_base) return true;
    const char* env = getenv("GFO_REF_ARENA_GIB");
    for (size_t gib = env ? (size_t)atol(env) : 64; gib >= 1; gib /= 2) {
        void* p = mmap(NULL, gib << 30, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p != MAP_FAILED) {
            g_base = (char*)p;
            g_cap = gib << 30;
            return true;
        }
    }
    return false;
}

void* allocate(size_t n)
{
    if (g_active) {
        if (n == kListNode) g_stats[1]++;
        if (!g_system) {
            const size_t a = (n + 15) & ~(size_t)15;
            if (a > g_cap - g_used) {
                g_stats[4]++;
                return NULL;
            }
            void* p = g_base + g_used;
            g_used += a;
            g_stats[0]++;
            g_stats[3] = (long long)g_used;
            return p;
        }
        g_stats[2]++;
    }
    return malloc(n ? n : 1);
}

void release(void* p)
{
    if (p && !in_arena(p)) free(p);
}

// Starts a call: what the previous call left in the arena is dropped first (the pyramid views), then the arena starts over.
struct Call {
    explicit Call(ORB_SLAM2::ORBextractor* ex)
    {
        for (size_t l = 0; l < ex->mvImagePyramid.size(); l++) ex->mvImagePyramid[l] = cv::Mat();
        if (g_used) madvise(g_base, g_used, MADV_DONTNEED);
        g_used = 0;
        memset(g_stats, 0, sizeof g_stats);
        cv_fast_log_clear();
        g_active = true;
    }
    ~Call() { g_active = false; }
};
}  // namespace

void* operator new(size_t n)
{
    void* p = allocate(n);
    if (!p) throw std::bad_alloc();
    return p;
}
void* operator new[](size_t n) { return operator new(n); }
void* operator new(size_t n, const std::nothrow_t&) noexcept { return allocate(n); }
void* operator new[](size_t n, const std::nothrow_t&) noexcept { return allocate(n); }
void operator delete(void* p) noexcept { release(p); }
void operator delete[](void* p) noexcept { release(p); }
void operator delete(void* p, size_t) noexcept { release(p); }
void operator delete[](void* p, size_t) noexcept { release(p); }
void operator delete(void* p, const std::nothrow_t&) noexcept { release(p); }
void operator delete[](void* p, const std::nothrow_t&) noexcept { release(p); }

namespace
{
// the protected tables (ORBextractor.h:149-151) through a derived class
struct Probe : ORB_SLAM2::ORBextractor {
    Probe(int nf, float sf, int nl, int ini, int mn) : ORB_SLAM2::ORBextractor(nf, sf, nl, ini, mn) {}
    const std::vector<int>& features_per_level() const { return mnFeaturesPerLevel; }
    const std::vector<int>& umax_table() const { return umax; }
    const std::vector<cv::Point>& pattern_table() const { return pattern; }
};

struct Handle {
    Probe* ex;
    std::vector<orc_keypoint> kp;
    std::vector<uint8_t> desc;
};

// DistributeOctTree indexes vpIniNodes[kp.pt.x / hX] with nIni = round((maxX - minX) / (maxY - minY)) nodes (ORBextractor.cc:543-569).
// Where that rounds to 0 and the level has FAST cells, the first corner found writes through an empty vector: undefined behaviour
// (a crash) rather than a result.  Such calls are refused before they run; a negative count throws and is caught (rc -1).
bool would_index_no_nodes(const ORB_SLAM2::ORBextractor* ex, int w, int h)
{
    ORB_SLAM2::ORBextractor* e = const_cast<ORB_SLAM2::ORBextractor*>(ex);
    const std::vector<float> inv = e->GetInverseScaleFactors();
    for (int l = 0; l < e->GetLevels(); l++) {
        const int cols = cvRound((float)w * inv[l]), rows = cvRound((float)h * inv[l]);   // ComputePyramid's level size (:1181)
        const int minB = 16, maxX = cols - 16, maxY = rows - 16;                        // ComputeKeyPointsOctTree (:773-776)
        const float width = (float)(maxX - minB), height = (float)(maxY - minB);
        const bool cells = width / 30.f >= 1.f && height / 30.f >= 1.f;                  // nCols, nRows >= 1 (:782-783)
        const float ratio = (float)(maxX - minB) / (maxY - minB);
        if (cells && std::isfinite(ratio) && std::round(ratio) == 0.f) return true;
    }
    return false;
}

cv::Mat image_of(const uint8_t* img, int w, int h, int stride)
{
    if (!img || w <= 0 || h <= 0) return cv::Mat();
    return cv::Mat(h, w, CV_8UC1, (void*)img, (size_t)stride);
}
}  // namespace

EXPORT void* ref_ex_create(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th)
{
    if (nlevels < 1 || nlevels > 32) return NULL;
    Handle* h = new Handle();
    h->ex = new Probe(nfeatures, scale_factor, nlevels, ini_th, min_th);
    return h;
}

EXPORT void ref_ex_destroy(void* p)
{
    Handle* h = (Handle*)p;
    if (!h) return;
    for (size_t l = 0; l < h->ex->mvImagePyramid.size(); l++) h->ex->mvImagePyramid[l] = cv::Mat();
    delete h->ex;
    delete h;
}

// scale[n], inv_scale[n], sigma2[n], inv_sigma2[n], features[n], umax[16], pattern[512 * 2]; returns nlevels
EXPORT int ref_ex_tables(void* p, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2, int* features, int* umax, int* pattern)
{
    Probe* ex = ((Handle*)p)->ex;
    const int n = ex->GetLevels();
    const std::vector<float> a = ex->GetScaleFactors(), b = ex->GetInverseScaleFactors(), c = ex->GetScaleSigmaSquares(),
                             d = ex->GetInverseScaleSigmaSquares();
    memcpy(scale, a.data(), sizeof(float) * n);
    memcpy(inv_scale, b.data(), sizeof(float) * n);
    memcpy(sigma2, c.data(), sizeof(float) * n);
    memcpy(inv_sigma2, d.data(), sizeof(float) * n);
    memcpy(features, ex->features_per_level().data(), sizeof(int) * n);
    memcpy(umax, ex->umax_table().data(), sizeof(int) * 16);
    for (int i = 0; i < 512; i++) {
        pattern[2 * i] = ex->pattern_table()[i].x;
        pattern[2 * i + 1] = ex->pattern_table()[i].y;
    }
    return n;
}

// ORBextractor::operator()(image, noArray(), keypoints, descriptors).  Returns the keypoint count, or -1 where the reference threw
// (a std::vector sized from a negative node count, ORBextractor.cc:549, on levels whose border-less extent is negative), -2 where
// the arena ran out, -4 where it would index an empty node vector (would_index_no_nodes).  The results stay in the handle for
// ref_ex_result.
EXPORT int ref_ex_extract(void* p, const uint8_t* img, int w, int h, int stride)
{
    Handle* hd = (Handle*)p;
    if (!reserve()) return -2;
    if (img && w > 0 && h > 0 && would_index_no_nodes(hd->ex, w, h)) return -4;
    int rc = 0;
    {
        Call call(hd->ex);
        std::vector<cv::KeyPoint> kps;
        cv::Mat desc;
        try {
            (*hd->ex)(image_of(img, w, h, stride), cv::Mat(), kps, desc);
        } catch (const std::bad_alloc&) {
            rc = g_stats[4] ? -2 : -1;
        } catch (...) {
            rc = -1;
        }
        g_active = false;   // the copies below are the shim's, not the reference's
        hd->kp.clear();
        hd->desc.clear();
        if (rc == 0) {
            hd->kp.resize(kps.size());
            for (size_t i = 0; i < kps.size(); i++) {
                const cv::KeyPoint& k = kps[i];
                orc_keypoint q = {k.pt.x, k.pt.y, k.size, k.angle, k.response, k.octave, k.class_id};
                hd->kp[i] = q;
            }
            if (!kps.empty()) {
                if (desc.rows != (int)kps.size() || desc.cols != 32) return -3;
                hd->desc.resize(kps.size() * 32);
                for (int i = 0; i < desc.rows; i++) memcpy(&hd->desc[(size_t)i * 32], desc.ptr(i), 32);
            }
            rc = (int)kps.size();
        }
    }
    return rc;
}

EXPORT void ref_ex_result(void* p, orc_keypoint* kp, uint8_t* desc)
{
    Handle* h = (Handle*)p;
    if (!h->kp.empty()) memcpy(kp, h->kp.data(), sizeof(orc_keypoint) * h->kp.size());
    if (!h->desc.empty()) memcpy(desc, h->desc.data(), h->desc.size());
}

// ORBextractor::ComputePyramid alone (public in this reference, ORBextractor.h:127); 0, or -1 where it threw
EXPORT int ref_ex_compute_pyramid(void* p, const uint8_t* img, int w, int h, int stride)
{
    Handle* hd = (Handle*)p;
    if (!reserve()) return -2;
    Call call(hd->ex);
    try {
        hd->ex->ComputePyramid(image_of(img, w, h, stride));
    } catch (...) {
        return -1;
    }
    return 0;
}

// the level of the last call (unblurred), as mvImagePyramid[level] holds it; padded: with the 19-px frame of its parent allocation
EXPORT int ref_ex_level_size(void* p, int level, int* w, int* h)
{
    Probe* ex = ((Handle*)p)->ex;
    if (level < 0 || level >= ex->GetLevels() || !ex->mvImagePyramid[level].data) return -1;
    *w = ex->mvImagePyramid[level].cols;
    *h = ex->mvImagePyramid[level].rows;
    return 0;
}

EXPORT int ref_ex_get_level(void* p, int level, int padded, uint8_t* out, int out_stride)
{
    Probe* ex = ((Handle*)p)->ex;
    if (level < 0 || level >= ex->GetLevels() || !ex->mvImagePyramid[level].data) return -1;
    const cv::Mat& m = ex->mvImagePyramid[level];
    const uint8_t* src = m.data;
    int w = m.cols, h = m.rows;
    if (padded) {
        cv::Size whole;
        cv::Point ofs;
        m.locateROI(whole, ofs);
        if (ofs.x != 19 || ofs.y != 19 || whole.width != w + 38 || whole.height != h + 38) return -1;
        src -= 19 * m.step + 19;
        w = whole.width;
        h = whole.height;
    }
    for (int y = 0; y < h; y++) memcpy(out + (size_t)y * out_stride, src + (size_t)y * m.step, (size_t)w);
    return 0;
}

// the FAST log of the last call: calls[9 * i ...] = {level_w, level_h, x, y, w, h, threshold, first, count}; corners = {x, y, score}
EXPORT int ref_fast_log_size() { return cv_fast_log_size(); }
EXPORT int ref_fast_log_ncorners() { return cv_fast_log_ncorners(); }
EXPORT void ref_fast_log_get(int* calls, int* corners)
{
    memcpy(calls, cv_fast_log_calls(), sizeof(cv_fast_call) * (size_t)cv_fast_log_size());
    memcpy(corners, cv_fast_log_corners(), sizeof(int) * 3 * (size_t)cv_fast_log_ncorners());
}

EXPORT void ref_set_system_allocator(int on) { g_system = on != 0; }

// of the last call: {arena allocations, allocations of a std::list<ExtractorNode> node, malloc allocations, arena bytes, overflows}
EXPORT void ref_arena_stats(long long* out) { memcpy(out, g_stats, sizeof g_stats); }
EXPORT long long ref_list_node_size() { return (long long)kListNode; }
