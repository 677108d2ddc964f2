// gfo_undistort.hip -- Frame::UndistortKeyPoints / UndistortKeyPointsStereo (src/Frame.cc:670-756) on the device:
// cv::undistortPoints of every keypoint of a batch, written next to the keypoints as mvKeysUn (gfo_ctx::d_kp_un).
// The per-point arithmetic is include/gfo_undistort.h (OpenCV 3.4.1's, in double, DESIGN.md 0 [OCV]).
//
// One lane per keypoint, the two cameras as a kernel argument.  The work is tiny (at most a few thousand points of ~60 double
// operations and five divisions each); what it costs is one more launch at the end of the per-frame chain.  gfo_api.hip reaches
// this file only through gfo_ctx::undistort, which gfo_ctx_set_camera installs, and gfo_kernels_undistort_hook.
#include "gfo_internal.h"

#include <math.h>
#include <stdarg.h>

#define UD_TRY(c, expr)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return gfo_fail((c), GFO_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define UD_BLOCK 64   // one wave per workgroup: a frame's ~1000 keypoints spread over ~16 CUs instead of 4

struct UdCams {
    GfoUndistCam cam[2];   // [0] left / mono, [1] right (images 2k + 1) when two_cams
    int two_cams;
};

// image blockIdx.y of the batch: keypoint i (below the image's count) -> its undistorted copy; only x, y change
__global__ __launch_bounds__(UD_BLOCK) void k_undistort_kp(const gfo_keypoint* __restrict__ kp, gfo_keypoint* __restrict__ kp_un,
                                                            const int* __restrict__ cnt, int ks, UdCams cams)
{
    const int img = blockIdx.y;
    const int i = blockIdx.x * UD_BLOCK + threadIdx.x;
    const int n = cnt[img] < ks ? cnt[img] : ks;
    if (i >= n) return;
    const size_t o = (size_t)img * ks + i;
    gfo_keypoint k = kp[o];
    const GfoUndistCam* c = &cams.cam[cams.two_cams ? (img & 1) : 0];
    gfo_undistort_point(c, k.x, k.y, &k.x, &k.y);
    kp_un[o] = k;
}

// n (x, y) pairs in place (gfo_undistort_points)
__global__ __launch_bounds__(UD_BLOCK) void k_undistort_xy(float2* __restrict__ xy, int n, GfoUndistCam cam)
{
    const int i = blockIdx.x * UD_BLOCK + threadIdx.x;
    if (i >= n) return;
    float2 p = xy[i];
    gfo_undistort_point(&cam, p.x, p.y, &p.x, &p.y);
    xy[i] = p;
}

// gfo_ctx::undistort: after the descriptors of an extraction of nimg images (extract_launches, gfo_api.hip)
static int launch_undistort(gfo_ctx* c, int nimg)
{
    if (!c->d_kp_un) return gfo_fail(c, GFO_ERR_STATE, "no buffer for the undistorted keypoints");
    UdCams cams{};
    cams.cam[0] = c->cam[0];
    cams.cam[1] = c->cam[c->n_cams > 1 ? 1 : 0];
    cams.two_cams = c->n_cams > 1;
    const int ks = c->g.kp_stride;
    gfo_prof_begin(c, ST_UNDISTORT);
    GFO_LAUNCH(c, k_undistort_kp, dim3((unsigned)((ks + UD_BLOCK - 1) / UD_BLOCK), (unsigned)nimg), dim3(UD_BLOCK), 0, c->stream, c->d_kp,
               c->d_kp_un, c->d_kp_cnt, ks, cams);
    gfo_prof_end(c);
    return GFO_OK;
}

static void gfo_kernels_undistort(std::vector<const void*>& v)
{
    v.push_back((const void*)k_undistort_kp);
    v.push_back((const void*)k_undistort_xy);
}
// (gfo_preload_kernels runs at the first gfo_ctx_create, long after the library's static initialisers)
static const struct UdRegister {
    UdRegister() { gfo_kernels_undistort_hook = gfo_kernels_undistort; }
} ud_register;

// ---- host side -------------------------------------------------------------------------------------------------------------------
static bool finite_all(const float* v, int n)
{
    for (int i = 0; i < n; i++)
        if (!isfinite(v[i])) return false;
    return true;
}

static int validate(gfo_ctx* c, const gfo_camera* g, const char* which)
{
    if (g->n_dist != 4 && g->n_dist != 5 && g->n_dist != 8)
        return gfo_fail(c, GFO_ERR_INVALID, "%s camera: n_dist %d (4, 5 or 8 coefficients; fisheye and 12/14-coefficient models are not supported)", which, g->n_dist);
    if ((g->has_R != 0 && g->has_R != 1) || (g->has_P != 0 && g->has_P != 1))
        return gfo_fail(c, GFO_ERR_INVALID, "%s camera: has_R / has_P must be 0 or 1", which);
    if (!finite_all(g->K, 9) || !finite_all(g->D, g->n_dist) || (g->has_R && !finite_all(g->R, 9)) || (g->has_P && !finite_all(g->P, 12)))
        return gfo_fail(c, GFO_ERR_INVALID, "%s camera: a value is not finite", which);
    if (g->K[0] == 0.0f || g->K[4] == 0.0f) return gfo_fail(c, GFO_ERR_INVALID, "%s camera: fx and fy must not be 0", which);
    return GFO_OK;
}

// cvUndistortPointsInternal's set-up (undistort.cpp): the float matrices widened to double (cvConvert), RR = P[:, :3] * R by cvMatMul --
// each entry (PP[i][0] * R[0][j] + PP[i][1] * R[1][j]) + PP[i][2] * R[2][j], left to right (cv::gemm's 3x3 path), times alpha = 1
static void prepare(const gfo_camera* g, GfoUndistCam* u)
{
    double A[9];
    for (int i = 0; i < 9; i++) A[i] = (double)g->K[i];
    u->fx = A[0];
    u->fy = A[4];
    u->ifx = 1. / u->fx;
    u->ify = 1. / u->fy;
    u->cx = A[2];
    u->cy = A[5];
    for (int i = 0; i < 8; i++) u->k[i] = i < g->n_dist ? (double)g->D[i] : 0.0;
    double R[9];
    for (int i = 0; i < 9; i++) R[i] = g->has_R ? (double)g->R[i] : (i % 4 == 0 ? 1.0 : 0.0);
    if (g->has_P) {
        double PP[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) PP[i * 3 + j] = (double)g->P[i * 4 + j];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double t = PP[i * 3 + 0] * R[0 * 3 + j] + PP[i * 3 + 1] * R[1 * 3 + j] + PP[i * 3 + 2] * R[2 * 3 + j];
                u->rr[i * 3 + j] = t * 1.0;
            }
    } else {
        for (int i = 0; i < 9; i++) u->rr[i] = R[i];
    }
}

extern "C" int gfo_ctx_set_camera(gfo_ctx* c, const gfo_camera* left, const gfo_camera* right)
{
    if (!c) return GFO_ERR_INVALID;
    if (!left && right) return gfo_fail(c, GFO_ERR_INVALID, "a right camera without a left one");
    if (left)
        if (int rc = validate(c, left, "left")) return rc;
    if (right)
        if (int rc = validate(c, right, "right")) return rc;
    const int n = left ? (right ? 2 : 1) : 0;
    if (n == c->n_cams && (n < 1 || memcmp(&c->cam_abi[0], left, sizeof(gfo_camera)) == 0) &&
        (n < 2 || memcmp(&c->cam_abi[1], right, sizeof(gfo_camera)) == 0))
        return GFO_OK;   // the cameras the context already has
    UD_TRY(c, hipSetDevice(c->device));
    UD_TRY(c, hipStreamSynchronize(c->stream));   // nothing submitted may still read the buffers below
    if (n > 0 && c->planned && !c->d_kp_un)
        UD_TRY(c, hipMalloc(&c->d_kp_un, (size_t)c->cap_batch * c->g.kp_stride * sizeof(gfo_keypoint)));
    // (from here on nothing can fail)
    GfoUndistCam cams[2]{};
    // Frame::UndistortKeyPoints: undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) -- P = K.  (Frame passes no R there; an R the
    // caller does give is applied, RR = K * R, as undistortPoints(K, D, R, K) would -- include/gfo.h says so.)
    if (left && !right && !left->has_P) {
        gfo_camera m = *left;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) m.P[i * 4 + j] = j < 3 ? m.K[i * 3 + j] : 0.0f;
        m.has_P = 1;
        prepare(&m, &cams[0]);
    } else if (left) {
        prepare(left, &cams[0]);
    }
    if (right) prepare(right, &cams[1]);
    c->cam[0] = cams[0];
    c->cam[1] = cams[1];
    memset(c->cam_abi, 0, sizeof c->cam_abi);
    if (left) c->cam_abi[0] = *left;
    if (right) c->cam_abi[1] = *right;
    c->n_cams = n;
    c->has_camera = n > 0;
    // the Frame gates (Frame.cc:672-677, 726-730): the LEFT camera's k1 == 0 leaves every keypoint as extracted (mvKeysUn = mvKeys)
    c->undistort = n > 0 && left->D[0] != 0.0f ? launch_undistort : nullptr;
    if (c->graph_exec) {   // a captured launch sequence (GFO_GRAPH=1) has the old cameras in it
        (void)hipGraphExecDestroy(c->graph_exec);
        c->graph_exec = nullptr;
    }
    c->have_batch = c->have_stereo = c->have_projection = false;   // the last batch's mvKeysUn belonged to the old cameras
    return GFO_OK;
}

extern "C" int gfo_undistort_points(gfo_ctx* c, const gfo_camera* cam, const float* xy, int n, float* out_xy)
{
    if (!c || !cam || n < 0 || (n > 0 && (!xy || !out_xy))) return c ? gfo_fail(c, GFO_ERR_INVALID, "bad argument") : GFO_ERR_INVALID;
    if (int rc = validate(c, cam, "the")) return rc;
    if (n == 0) return GFO_OK;
    GfoUndistCam u{};
    prepare(cam, &u);
    const size_t bytes = 8 * (size_t)n;
    UD_TRY(c, hipSetDevice(c->device));
    if (bytes > c->un_pts_bytes) {
        UD_TRY(c, hipStreamSynchronize(c->stream));
        if (c->d_un_pts) (void)hipFree(c->d_un_pts);
        c->d_un_pts = nullptr;
        c->un_pts_bytes = 0;
        UD_TRY(c, hipMalloc(&c->d_un_pts, bytes));
        c->un_pts_bytes = bytes;
    }
    UD_TRY(c, hipMemcpyAsync(c->d_un_pts, xy, bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_undistort_xy, dim3((unsigned)((n + UD_BLOCK - 1) / UD_BLOCK)), dim3(UD_BLOCK), 0, c->stream, (float2*)c->d_un_pts, n, u);
    UD_TRY(c, hipGetLastError());
    UD_TRY(c, hipMemcpyAsync(out_xy, c->d_un_pts, bytes, hipMemcpyDeviceToHost, c->stream));
    UD_TRY(c, hipStreamSynchronize(c->stream));
    return GFO_OK;
}
