"""Frame::ComputeImageBounds / ComputeImageBoundsStereo (src/Frame.cc:760-830) on top of the device's cv::undistortPoints
(ORBextractor.undistort_points, gfo_undistort_points)."""
import numpy as np

_INT_MAX = np.float32(2147483647)    # mnMinX = INT_MAX: the static float members take the int's float value
_INT_MIN = np.float32(-2147483648)


def image_bounds(extractor, cols, rows, K, D, R=None, P=None):
    """(mnMinX, mnMinY, mnMaxX, mnMaxY) -- the order of gfo_frame_bounds / FrameBounds -- of an image of cols x rows pixels.
    R = P = None: ComputeImageBounds (cv::undistortPoints(corners, K, D, cv::Mat(), K)); R, P given: ComputeImageBoundsStereo
    (undistortPoints(corners, K, D, R, P)).  k1 == 0: the image itself (the reference's gate)."""
    D = np.asarray(D, np.float32).reshape(-1)
    if D[0] == 0.0:
        return 0.0, 0.0, float(np.float32(cols)), float(np.float32(rows))
    c, r = np.float32(cols), np.float32(rows)
    c2, r2 = np.float32(float(cols) / 2.0), np.float32(float(rows) / 2.0)
    z = np.float32(0.0)
    pts = np.array([[z, z], [c, z], [z, r], [c, r], [z, r2], [c2, z], [c2, r], [c, r2]], np.float32)
    if R is None and P is None:
        P = np.asarray(K, np.float32).reshape(3, 3)
    out = extractor.undistort_points(pts, K, D, R, P)
    min_x, max_x, min_y, max_y = _INT_MAX, _INT_MIN, _INT_MAX, _INT_MIN
    for x, y in out:
        if min_x > x:
            min_x = np.floor(x)
        if min_y > y:
            min_y = np.floor(y)
        if max_x < x:
            max_x = np.ceil(x)
        if max_y < y:
            max_y = np.ceil(y)
    return float(min_x), float(min_y), float(max_x), float(max_y)
