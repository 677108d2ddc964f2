"""CPU checks of the undistortion's independent statement (tests/undistort_ref.py) and of the host-side pieces of the feature that need no
device: known answers of cv::undistortPoints, the Frame gates, the rig the GPU tests use, the Python camera record."""
import ctypes

import numpy as np
import pytest

import undistort_ref as U


def _grid(w=752, h=480, step=16, margin=40):
    xs = np.arange(-margin, w + margin + 1, step, dtype=np.float32)
    ys = np.arange(-margin, h + margin + 1, step, dtype=np.float32)
    gx, gy = np.meshgrid(xs, ys)
    return np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)


def _kps(xy):
    kp = np.zeros(len(xy), [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                            ("class_id", "<i4")])
    kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
    kp["size"], kp["angle"], kp["response"], kp["octave"], kp["class_id"] = 31.0, 12.5, 0.25, 2, -1
    return kp


def test_zero_distortion_identity_rotation_and_p_equal_k_is_the_identity_to_the_bit():
    xy = _grid()        # (no coordinate is exactly 0: (0 - cx) * (1 / fx) * fx + cx leaves ~1e-14 there, not 0)
    assert (xy != 0).all()
    for n in (4, 5, 8):
        out = U.undistort_points(xy, U.K_L, np.zeros(n, np.float32), np.eye(3, dtype=np.float32), U.K_L)
        assert out.tobytes() == xy.tobytes(), f"{n} coefficients"


def test_mono_gate_copies_the_keypoints_when_k1_is_zero():
    kp = _kps(_grid())
    D = U.D_L.copy()
    D[0] = 0.0      # k2, p1, p2 stay: the reference gates on k1 alone (Frame.cc:726)
    assert U.undistort_mono(kp, U.K_L, D).tobytes() == kp.tobytes()
    D[0] = -0.0
    assert U.undistort_mono(kp, U.K_L, D).tobytes() == kp.tobytes()
    moved = U.undistort_mono(kp, U.K_L, U.D_L)
    assert moved.tobytes() != kp.tobytes()
    for f in ("size", "angle", "response", "octave", "class_id"):      # only pt changes
        assert (moved[f] == kp[f]).all()


def test_stereo_gate_follows_the_left_camera_only():
    kl, kr = _kps(_grid()), _kps(_grid()[::-1].copy())
    Dl = U.D_L.copy()
    Dl[0] = 0.0
    ul, ur = U.undistort_stereo(kl, kr, (U.K_L, Dl, U.R_L, U.P_L), (U.K_R, U.D_R, U.R_R, U.P_R))
    assert ul.tobytes() == kl.tobytes() and ur.tobytes() == kr.tobytes()          # R, P given and the right k1 != 0: still unchanged
    Dr = U.D_R.copy()
    Dr[0] = 0.0
    ul, ur = U.undistort_stereo(kl, kr, (U.K_L, U.D_L, U.R_L, U.P_L), (U.K_R, Dr, U.R_R, U.P_R))
    assert ul.tobytes() != kl.tobytes() and ur.tobytes() != kr.tobytes()          # a right k1 of 0 gates nothing (R, P still apply)


@pytest.mark.parametrize("D", [U.D_L, U.D5, U.D8], ids=["4", "5", "8"])
def test_round_trip_near_the_centre(D):
    """sanity only: five fixed iterations converge near the centre (not at the corners, where OpenCV's answer is what it is)"""
    rng = np.random.default_rng(1)
    xn = rng.uniform(-0.3, 0.3, (500, 2))
    xd = U.distort_points(xn, D)
    K = U.K_L.astype(np.float64)
    px = np.stack([xd[:, 0] * K[0, 0] + K[0, 2], xd[:, 1] * K[1, 1] + K[1, 2]], axis=1).astype(np.float32)
    back = U.undistort_points(px, U.K_L, D, None, U.K_L).astype(np.float64)
    want = np.stack([xn[:, 0] * K[0, 0] + K[0, 2], xn[:, 1] * K[1, 1] + K[1, 2]], axis=1)
    assert np.abs(back - want).max() < 2e-3      # px; float32 pixel inputs carry ~3e-5 px of rounding


def test_the_rig_moves_edge_keypoints_out_of_the_image():
    """the calibration of the GPU tests sends keypoints near the edges to y < 0, y > rows - 1 and x < 0 (mnMinX of the association), so
    that the association's row guard (Frame.cc:1210) and the projection bounds are exercised"""
    pts = np.array([[25, 25], [726, 25], [25, 455], [726, 455], [376, 22], [376, 458], [22, 240]], np.float32)
    ul = U.undistort_points(pts, U.K_L, U.D_L, U.R_L, U.P_L)
    assert (ul[:, 1] < 0).any() and (ul[:, 1] > 479).any() and (ul[:, 0] < 0).any()
    ur = U.undistort_points(pts, U.K_R, U.D_R, U.R_R, U.P_R)
    assert (ur[:, 1] < 0).any() and (ur[:, 1] > 479).any()
    # R and P shift the rectified frame: the right camera's -bf in P[0, 3] does not enter (only P's left 3x3 is used)
    assert U.prepare(U.K_R, U.D_R, U.R_R, U.P_R)["RR"][0, 0] != U.prepare(U.K_R, U.D_R, None, None)["RR"][0, 0]


def test_camera_record_layout_and_shapes():
    from gf_orb_slam2_amd._lib import CameraC, make_camera
    assert ctypes.sizeof(CameraC) == 4 * (9 + 8 + 1 + 9 + 12 + 2)
    cam = make_camera(U.K_R, U.D_R, U.R_R, U.P_R)
    assert cam.n_dist == 4 and cam.has_R == 1 and cam.has_P == 1 and cam.P[3] == np.float32(-U.BF)
    cam = make_camera(U.K_L, U.D8, None, U.K_L)          # P given as 3x3 (Frame's mono call passes K)
    assert cam.n_dist == 8 and cam.has_R == 0 and cam.has_P == 1 and cam.P[3] == 0.0 and cam.P[2] == np.float32(U.K_L[0, 2])
    with pytest.raises(ValueError):
        make_camera(np.eye(2), U.D_L)
    with pytest.raises(ValueError):
        make_camera(U.K_L, np.zeros(12))                 # 12/14-coefficient models: refused
    with pytest.raises(ValueError):
        make_camera(U.K_L, U.D_L, None, np.zeros((2, 4)))


def test_image_bounds_gate_needs_no_device():
    """ComputeImageBounds(Stereo) with k1 == 0: the image itself, no undistortion called"""
    import gf_orb_slam2_amd as G
    D = U.D_L.copy()
    D[0] = 0.0
    assert G.image_bounds(None, 752, 480, U.K_L, D) == (0.0, 0.0, 752.0, 480.0)
    assert G.image_bounds(None, 752, 480, U.K_L, D, U.R_L, U.P_L) == (0.0, 0.0, 752.0, 480.0)
