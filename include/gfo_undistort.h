/* gfo_undistort.h -- cv::undistortPoints (OpenCV 3.4.1, radial-tangential model) for one point, shared by the HIP kernel and the host.
 *
 * The reference maps every keypoint into the undistorted (stereo: rectified) frame with
 *   cv::undistortPoints(pts, K, D, R, P)            Frame::UndistortKeyPointsStereo, src/Frame.cc:670-722
 *   cv::undistortPoints(pts, K, D, cv::Mat(), K)    Frame::UndistortKeyPoints, :724-756; ComputeImageBounds, :760-830
 * i.e. cvUndistortPointsInternal (modules/imgproc/src/undistort.cpp): everything in double, the tilt step with the identity matrix,
 * five fixed-point iterations of the inverse distortion (TermCriteria(COUNT, 5): no early exit), then the projection by
 * RR = P[:, :3] * R.  DESIGN.md 0 states it as an [OCV] restatement (recalled, not pinned against a build of OpenCV).
 *
 * Every expression below is written in OpenCV's order and evaluated left to right; build with -ffp-contract=off (the library does)
 * so that nothing is fused.  Where OpenCV multiplies by 0 or 1 (the identity tilt matrix, the thin-prism terms of a model with at most
 * eight coefficients) the operation is kept: it can change the sign of a zero, and the outputs are compared bit for bit.
 */
#ifndef GFO_UNDISTORT_H
#define GFO_UNDISTORT_H

/* one camera as the per-point arithmetic needs it (gfo_undistort_prepare fills it from a gfo_camera) */
typedef struct {
    double fx, fy, cx, cy;  /* A[0][0], A[1][1], A[0][2], A[1][2]                                       */
    double ifx, ify;        /* 1./fx, 1./fy: OpenCV multiplies by the reciprocals                        */
    double k[8];            /* k1 k2 p1 p2 k3 k4 k5 k6; coefficients the camera does not give are 0      */
    double rr[9];           /* RR row-major                                                              */
} GfoUndistCam;

#if defined(__HIPCC__) || defined(__HIP__)
#define GFO_UD_HD __host__ __device__
#else
#define GFO_UD_HD
#endif

/* (u, v) pixel of the distorted image -> (*ou, *ov) in the frame of RR (cvUndistortPointsInternal's loop body, float in, float out) */
static GFO_UD_HD inline void gfo_undistort_point(const GfoUndistCam* c, float u, float v, float* ou, float* ov)
{
    const double* k = c->k;
    double x = (double)u, y = (double)v;
    x = (x - c->cx) * c->ifx;
    y = (y - c->cy) * c->ify;
    /* cv::Vec3d vecUntilt = invMatTilt * cv::Vec3d(x, y, 1) with invMatTilt = Matx33d::eye(): Matx_MatMulOp sums from 0 in column order */
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    t0 += 1.0 * x; t0 += 0.0 * y; t0 += 0.0 * 1.0;
    t1 += 0.0 * x; t1 += 1.0 * y; t1 += 0.0 * 1.0;
    t2 += 0.0 * x; t2 += 0.0 * y; t2 += 1.0 * 1.0;
    const double inv_proj = t2 != 0.0 ? 1. / t2 : 1.0;
    const double x0 = inv_proj * t0, y0 = inv_proj * t1;
    x = x0;
    y = y0;
    /* the thin-prism coefficients k[8..11] of a 12/14-coefficient model are 0 here (such models are refused) */
    const double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        const double dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 * r2;
        const double dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + s3 * r2 + s4 * r2 * r2;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    const double* R = c->rr;
    const double xx = R[0] * x + R[1] * y + R[2];
    const double yy = R[3] * x + R[4] * y + R[5];
    const double ww = 1. / (R[6] * x + R[7] * y + R[8]);
    *ou = (float)(xx * ww);
    *ov = (float)(yy * ww);
}

#endif /* GFO_UNDISTORT_H */
