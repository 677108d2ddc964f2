"""An independent CPU statement of cv::undistortPoints (OpenCV 3.4.1, radial-tangential model) and of the Frame gates around it
(src/Frame.cc:670-756), in numpy float64 -- what tests/test_gpu_undistort.py compares the device with, bit for bit.

numpy's float64 elementwise operations are IEEE operations, each rounded once, never fused: every expression below is written as a
sequence of such operations in the order cvUndistortPointsInternal evaluates it (left to right), so the result is the double
computation of the C code.  DESIGN.md 0 states the arithmetic ([OCV]: recalled, not pinned against a build of OpenCV)."""
import numpy as np

# EuRoC-magnitude stereo rig (cam0 / cam1 of the MH sequences in round numbers; the reference ships no settings file for it).  The
# right camera's P carries -bf in P[0, 3]; R is a fraction of a degree off the identity.
K_L = np.array([[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]], np.float32)
D_L = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], np.float32)
K_R = np.array([[457.587, 0.0, 379.999], [0.0, 456.134, 255.238], [0.0, 0.0, 1.0]], np.float32)
D_R = np.array([-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05], np.float32)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (rz @ ry @ rx).astype(np.float32)


R_L = _rot(0.0031, -0.0044, 0.0012)
R_R = _rot(0.0027, 0.0061, -0.0009)
FX_P, BF = 435.2047, 47.90639
P_L = np.array([[FX_P, 0.0, 367.2, 0.0], [0.0, FX_P, 252.2, 0.0], [0.0, 0.0, 1.0, 0.0]], np.float32)
P_R = np.array([[FX_P, 0.0, 367.2, -BF], [0.0, FX_P, 252.2, 0.0], [0.0, 0.0, 1.0, 0.0]], np.float32)
# 5 and 8 coefficients (k3; k4 k5 k6 of the rational model), same magnitudes as the rig
D5 = np.array([-0.2834, 0.0740, 0.00019, 1.8e-05, -0.0081], np.float32)
D8 = np.array([-0.2834, 0.0740, 0.00019, 1.8e-05, -0.0081, 0.0123, -0.0021, 0.0007], np.float32)


def prepare(K, D, R=None, P=None):
    """cvUndistortPointsInternal's set-up: float matrices widened to double, RR = P[:, :3] * R (cvMatMul, each entry summed over k
    left to right), the reciprocals of fx, fy"""
    A = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    Dv = np.asarray(D, np.float32).astype(np.float64).reshape(-1)
    k = np.zeros(8)
    k[:Dv.size] = Dv
    Rm = np.eye(3) if R is None else np.asarray(R, np.float32).astype(np.float64).reshape(3, 3)
    if P is not None:
        PP = np.asarray(P, np.float32).astype(np.float64).reshape(3, -1)[:, :3]
        RR = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                t = PP[i, 0] * Rm[0, j]
                t = t + PP[i, 1] * Rm[1, j]
                t = t + PP[i, 2] * Rm[2, j]
                RR[i, j] = t
    else:
        RR = Rm.copy()
    fx, fy, cx, cy = A[0, 0], A[1, 1], A[0, 2], A[1, 2]
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, ifx=1.0 / fx, ify=1.0 / fy, k=k, RR=RR)


def undistort_points(xy, K, D, R=None, P=None):
    """cv::undistortPoints(xy, K, D, R, P) for float32 (n, 2) points -> float32 (n, 2); no Frame gate"""
    c = prepare(K, D, R, P)
    k, RR = c["k"], c["RR"]
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    x = xy[:, 0].astype(np.float64)
    y = xy[:, 1].astype(np.float64)
    x = (x - c["cx"]) * c["ifx"]
    y = (y - c["cy"]) * c["ify"]
    # Matx33d::eye() * Vec3d(x, y, 1): every row a sum from 0 over the columns
    t0 = ((0.0 + 1.0 * x) + 0.0 * y) + 0.0 * 1.0
    t1 = ((0.0 + 0.0 * x) + 1.0 * y) + 0.0 * 1.0
    t2 = ((0.0 + 0.0 * x) + 0.0 * y) + 1.0 * 1.0
    inv_proj = np.where(t2 != 0.0, 1.0 / t2, 1.0)
    x0 = inv_proj * t0
    y0 = inv_proj * t1
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + 0.0 * r2 + 0.0 * r2 * r2      # + k[8]*r2 + k[9]*r2*r2 (thin prism, 0)
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + 0.0 * r2 + 0.0 * r2 * r2      # + k[10]*r2 + k[11]*r2*r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    xx = RR[0, 0] * x + RR[0, 1] * y + RR[0, 2]
    yy = RR[1, 0] * x + RR[1, 1] * y + RR[1, 2]
    ww = 1.0 / (RR[2, 0] * x + RR[2, 1] * y + RR[2, 2])
    return np.stack([(xx * ww).astype(np.float32), (yy * ww).astype(np.float32)], axis=1)


def distort_points(xy_norm, D):
    """the forward model (normalised coordinates, float64): for the round-trip sanity check only"""
    k = np.zeros(8)
    Dv = np.asarray(D, np.float64).reshape(-1)
    k[:Dv.size] = Dv
    x, y = xy_norm[:, 0], xy_norm[:, 1]
    r2 = x * x + y * y
    radial = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = x * radial + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * radial + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    return np.stack([xd, yd], axis=1)


def undistort_keypoints(kp, K, D, R=None, P=None):
    """mvKeysUn from mvKeys of ONE camera, no gate: a copy of the keypoints with x, y replaced"""
    out = kp.copy()
    if len(kp):
        xy = undistort_points(np.stack([kp["x"], kp["y"]], axis=1), K, D, R, P)
        out["x"], out["y"] = xy[:, 0], xy[:, 1]
    return out


def undistort_mono(kp, K, D):
    """Frame::UndistortKeyPoints (Frame.cc:724-756): k1 == 0 -> mvKeys unchanged, else undistortPoints(K, D, cv::Mat(), K)"""
    if np.float32(np.asarray(D, np.float32).reshape(-1)[0]) == 0.0:
        return kp.copy()
    return undistort_keypoints(kp, K, D, None, K)


def undistort_stereo(kl, kr, left, right):
    """Frame::UndistortKeyPointsStereo (Frame.cc:670-722): left = (K, D, R, P), right likewise; the LEFT camera's k1 == 0 leaves both sides
    unchanged"""
    if np.float32(np.asarray(left[1], np.float32).reshape(-1)[0]) == 0.0:
        return kl.copy(), kr.copy()
    return undistort_keypoints(kl, *left), undistort_keypoints(kr, *right)
