"""GPU parity of the device undistortion (gfo_ctx_set_camera, gfo_undistort_points, gfo_extract_un, gfo_extract_stereo_un,
gfo_batch_fetch_un) and of every chain that reads mvKeysUn with a camera set, against the numpy statement of cv::undistortPoints
(tests/undistort_ref.py) feeding the CPU oracle.  Float outputs are compared by bit pattern, indices exactly."""
import ctypes as C

import numpy as np
import pytest

import undistort_ref as U
from conftest import synth_frame

pytestmark = pytest.mark.gpu

LEFT = (U.K_L, U.D_L, U.R_L, U.P_L)
RIGHT = (U.K_R, U.D_R, U.R_R, U.P_R)
MIN_X = 5.0      # mnMinX of the association: undistorted keypoints left of it exist on the rig (x < 0)


def _params(rows=480):
    import gf_orb_slam2_amd as G
    return G.StereoParams(rows, U.BF, U.BF / U.FX_P, MIN_X)


@pytest.fixture(scope="module")
def oracle_euroc(oracle, euroc_l, euroc_r):
    oe = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    kl, dl = oe(euroc_l)
    kr, dr = oe(euroc_r)
    return kl, dl, kr, dr, oe.scale_factors


@pytest.fixture
def ext():
    import gf_orb_slam2_amd as G
    e = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=8)
    yield e
    e.close()


def _bits_equal(a, b, what):
    assert a.shape == b.shape, what
    if a.tobytes() != b.tobytes():
        rows = (a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1)
        i = int(np.argmax(rows))
        raise AssertionError(f"{what}: {int(rows.sum())} of {len(a)} entries differ, first {i}: {a[i]} vs {b[i]}")


def _cmp_stereo(got, ref):
    assert got[0] == ref[0], f"nmatched {got[0]} vs {ref[0]}"
    for name, a, b in zip(("u_right", "depth", "best_dist", "best_idx"), got[1:], ref[1:]):
        assert a.tobytes() == b.tobytes(), name


def _dense_points():
    xs = np.linspace(-60.0, 812.0, 97, dtype=np.float32)
    ys = np.linspace(-45.0, 525.0, 71, dtype=np.float32)
    gx, gy = np.meshgrid(xs, ys)
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1)
    corners = np.array([[0, 0], [752, 0], [0, 480], [752, 480], [751.5, 479.5], [-0.0, -0.0], [376, 240], [367.215, 248.375]], np.float32)
    return np.concatenate([pts, corners]).astype(np.float32)


# ---- 1. arbitrary points -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [U.D_L, U.D5, U.D8], ids=["4", "5", "8"])
@pytest.mark.parametrize("form", ["K_only", "R_P", "P_only", "R_only"])
def test_undistort_points_against_the_statement(ext, D, form):
    R = U.R_L if form in ("R_P", "R_only") else None
    P = U.P_L if form in ("R_P", "P_only") else None
    xy = _dense_points()
    got = ext.undistort_points(xy, U.K_L, D, R, P)
    _bits_equal(got, U.undistort_points(xy, U.K_L, D, R, P), f"{len(D)} coefficients, {form}")


def test_undistort_points_mono_form_and_zero_distortion(ext):
    """Frame's mono call passes P = K; D = 0, R = I, P = K is the identity to the bit; k1 == 0 alone is not gated here (the caller's gate)"""
    xy = _dense_points()
    _bits_equal(ext.undistort_points(xy, U.K_L, U.D_L, None, U.K_L), U.undistort_points(xy, U.K_L, U.D_L, None, U.K_L), "mono")
    got = ext.undistort_points(xy, U.K_L, np.zeros(5, np.float32), np.eye(3), U.K_L)
    _bits_equal(got, U.undistort_points(xy, U.K_L, np.zeros(5, np.float32), np.eye(3), U.K_L), "zero distortion")
    away = (xy != 0).all(axis=1)      # a coordinate of exactly 0 comes back as ~1e-14: (0 - cx) / fx * fx + cx cancels in double
    _bits_equal(got[away], xy[away], "identity")
    D = U.D_L.copy()
    D[0] = 0.0
    _bits_equal(ext.undistort_points(xy, U.K_L, D, None, U.K_L), U.undistort_points(xy, U.K_L, D, None, U.K_L), "k1 = 0, ungated")


def test_image_bounds_restate_compute_image_bounds(ext):
    import gf_orb_slam2_amd as G
    for R, P in ((None, None), (U.R_L, U.P_L)):
        got = G.image_bounds(ext, 752, 480, U.K_L, U.D_L, R, P)
        pts = np.array([[0, 0], [752, 0], [0, 480], [752, 480], [0, 240], [376, 0], [376, 480], [752, 240]], np.float32)
        und = U.undistort_points(pts, U.K_L, U.D_L, R, U.K_L if P is None else P)
        want = (float(np.floor(und[:, 0].min())), float(np.floor(und[:, 1].min())), float(np.ceil(und[:, 0].max())), float(np.ceil(und[:, 1].max())))
        assert got == want
        assert got[0] < 0 and got[1] < 0 and got[2] > 752 and got[3] > 480      # barrel distortion: the undistorted image is larger


# ---- 2. single images and batches ------------------------------------------------------------------------------------------------
def test_extract_un_mono(ext, oracle, oracle_euroc, euroc_l):
    kl, dl = oracle_euroc[0], oracle_euroc[1]
    ext.set_camera(U.K_L, U.D_L)          # no P: Frame's mono call projects with K
    kp, ku, desc = ext.extract_un(euroc_l)
    assert kp.tobytes() == kl.tobytes() and (desc == dl).all(), "raw keypoints / descriptors must not change"
    _bits_equal(ku, U.undistort_mono(kl, U.K_L, U.D_L), "mvKeysUn")
    assert ku.tobytes() != kp.tobytes()
    # synthetic frame, 5 coefficients
    img = synth_frame(640, 480, 3)
    ko, do = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)(img)
    ext.set_camera(U.K_L, U.D5)
    kp, ku, desc = ext.extract_un(img)
    assert kp.tobytes() == ko.tobytes() and (desc == do).all()
    _bits_equal(ku, U.undistort_mono(ko, U.K_L, U.D5), "mvKeysUn, synthetic")
    # the mono gate: k1 == 0 -> mvKeysUn = mvKeys (the other coefficients notwithstanding)
    D = U.D_L.copy()
    D[0] = 0.0
    ext.set_camera(U.K_L, D)
    kp, ku, desc = ext.extract_un(img)
    assert ku.tobytes() == kp.tobytes() == ko.tobytes()


def test_extract_batch_and_batch_fetch_un(ext, oracle, oracle_euroc, euroc_l, euroc_r):
    """images 2k take the left camera, 2k + 1 the right one; raw outputs as without a camera"""
    kl, dl, kr, dr, _ = oracle_euroc
    s0, s1 = synth_frame(752, 480, 5), synth_frame(752, 480, 6)
    oe = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    ks0, ds0 = oe(s0)
    ks1, ds1 = oe(s1)
    ext.set_camera(*LEFT, right=RIGHT)
    kps, descs = ext.extract_batch([euroc_l, euroc_r, s0, s1])
    refs = [(kl, dl), (kr, dr), (ks0, ds0), (ks1, ds1)]
    for i, (k, d) in enumerate(refs):
        assert kps[i].tobytes() == k.tobytes() and (descs[i] == d).all(), f"image {i}"
        cam = LEFT if i % 2 == 0 else RIGHT
        _bits_equal(ext.batch_fetch_un(i), U.undistort_keypoints(k, *cam), f"mvKeysUn of image {i}")
        assert ext.batch_fetch(i)[0].tobytes() == k.tobytes()
    # 8 coefficients, left camera only (mono gate on the left camera, every image)
    ext.set_camera(U.K_L, U.D8, None, U.K_L)
    ext.extract_batch([s0, s1])
    _bits_equal(ext.batch_fetch_un(1), U.undistort_keypoints(ks1, U.K_L, U.D8, None, U.K_L), "8 coefficients")


# ---- 3. one stereo frame -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "rows", "keypoints"])
def test_extract_stereo_un_euroc(ext, oracle, oracle_euroc, euroc_l, euroc_r, form, monkeypatch):
    if form == "rows":
        monkeypatch.setenv("GFO_STEREO_ROWS", "5")
    elif form == "keypoints":
        monkeypatch.setenv("GFO_STEREO_ROWS", "0")
    kl, dl, kr, dr, sf = oracle_euroc
    ext.set_camera(*LEFT, right=RIGHT)
    p = _params()
    got = ext.extract_stereo_un(euroc_l, euroc_r, p)
    assert got[0].tobytes() == kl.tobytes() and (got[2] == dl).all() and got[3].tobytes() == kr.tobytes() and (got[5] == dr).all()
    ul, ur = U.undistort_stereo(kl, kr, LEFT, RIGHT)
    _bits_equal(got[1], ul, "mvKeysUn")
    _bits_equal(got[4], ur, "mvKeysRightUn")
    # the rig sends keypoints outside the rows (the row guard, Frame.cc:1210) and left of mnMinX
    assert (ul["y"] < 0).any() and (ul["y"] > 479).any() and (ul["x"] < MIN_X).any()
    assert (ur["y"] < 0).any() or (ur["y"] > 479).any()
    ref = oracle.stereo_match(ul, dl, ur, dr, sf, p.n_rows, p.mbf, p.mb, p.min_x)
    _cmp_stereo(got[6:], ref)
    assert ref[0] > 100
    # extract_stereo (no _un) on the same context associates the same undistorted arrays
    _cmp_stereo(ext.extract_stereo(euroc_l, euroc_r, p)[4:], ref)


def test_stereo_gate_on_the_left_camera(ext, oracle, oracle_euroc, euroc_l, euroc_r):
    kl, dl, kr, dr, sf = oracle_euroc
    D = U.D_L.copy()
    D[0] = 0.0
    ext.set_camera(U.K_L, D, U.R_L, U.P_L, right=RIGHT)
    p = _params()
    got = ext.extract_stereo_un(euroc_l, euroc_r, p)
    assert got[1].tobytes() == kl.tobytes() and got[4].tobytes() == kr.tobytes()
    _cmp_stereo(got[6:], oracle.stereo_match(kl, dl, kr, dr, sf, p.n_rows, p.mbf, p.mb, p.min_x))


# ---- 4. the device chain ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [1, 4])
def test_device_chain_with_a_camera(oracle, pairs):
    """extract_batch_device -> stereo_match_batch -> search_by_projection_batch with the rig set: every stage equals the oracle fed the
    undistorted keypoints (association and projection grid included)"""
    import torch
    import gf_orb_slam2_amd as G
    from gf_orb_slam2_amd.synth import synth_stereo_pair
    w, h = 752, 480
    frames = []
    for q in range(pairs):
        l, r = synth_stereo_pair(w, h, 60 + q)
        frames += [l, r]
    ext = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=2 * pairs)
    try:
        ext.set_camera(*LEFT, right=RIGHT)
        d_imgs = torch.from_numpy(np.stack(frames)).cuda()
        ext.extract_batch_device(d_imgs.data_ptr(), 2 * pairs, w, h)
        m = G.ORBmatcher(0.7, True, extractor=ext)
        p = _params(h)
        m.stereo_match_batch(p)
        sf = ext.GetScaleFactors()
        cap = ext.max_keypoints()
        kd, kun, urs = [], [], []
        for q in range(pairs):
            kl, dl = ext.batch_fetch(2 * q)
            kr, dr = ext.batch_fetch(2 * q + 1)
            ul, ur = U.undistort_stereo(kl, kr, LEFT, RIGHT)
            _bits_equal(ext.batch_fetch_un(2 * q), ul, f"pair {q} left")
            _bits_equal(ext.batch_fetch_un(2 * q + 1), ur, f"pair {q} right")
            ref = oracle.stereo_match(ul, dl, ur, dr, sf, p.n_rows, p.mbf, p.mb, p.min_x)
            got = m.stereo_fetch(q, cap)
            n = len(kl)
            _cmp_stereo((got[0], got[1][:n], got[2][:n], got[3][:n], got[4][:n]), ref)
            kd.append((kl, dl))
            kun.append(ul)
            urs.append(ref[1])
        # a map imitating pair 0's undistorted left keypoints
        rng = np.random.default_rng(9)
        M = 3000
        u0, d0 = kun[0], kd[0][1]
        src = rng.integers(0, len(u0), M)
        mpd = d0[src].copy()
        mpd[np.arange(M), rng.integers(0, 32, M)] ^= 1
        mps = np.zeros((pairs, M), G.MAP_POINT_DTYPE)
        for q in range(pairs):
            mps[q]["proj_x"] = u0["x"][src] + rng.normal(0, 2, M)
            mps[q]["proj_y"] = u0["y"][src] + rng.normal(0, 2, M)
            mps[q]["proj_xr"] = mps[q]["proj_x"] - rng.uniform(0, 30, M)
            mps[q]["level"] = u0["octave"][src]
            mps[q]["view_cos"] = 1.0
            mps[q]["flags"] = 5
        bounds = G.image_bounds(ext, w, h, *LEFT)
        m.map_upload(mpd)
        m.search_by_projection_batch(mps, bounds, th=3.0, stereo=True)
        for q in range(pairs):
            n = len(kun[q])
            ref = oracle.search_by_projection(kun[q], kd[q][1], urs[q], sf, bounds, mps[q], mpd, 3.0, 0.7, None)
            nm, out_mp, out_sc = m.projection_fetch(q, n)
            assert nm == ref[0], f"pair {q}"
            np.testing.assert_array_equal(out_mp[:n], ref[1])
            np.testing.assert_array_equal(out_sc[:n], ref[2])
        assert ref[0] > 100
    finally:
        ext.close()


# ---- 5. nothing changes without a camera -----------------------------------------------------------------------------------------
def test_no_camera_no_change(euroc_l, euroc_r):
    import gf_orb_slam2_amd as G
    p = _params()

    def run(e):
        r = e.extract_stereo(euroc_l, euroc_r, p)
        kps, descs = e.extract_batch([euroc_l, euroc_r, euroc_r])
        un = e.extract_un(euroc_r)
        return [np.asarray(x).tobytes() for x in r] + [k.tobytes() for k in kps] + [d.tobytes() for d in descs] + \
               [un[0].tobytes(), un[1].tobytes(), un[2].tobytes(), e.batch_fetch_un(0).tobytes()]

    a = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=4)
    before = run(a)
    assert before[-3] == before[-4]            # no camera: mvKeysUn = mvKeys
    a.set_camera(*LEFT, right=RIGHT)
    with_cam = a.extract_stereo(euroc_l, euroc_r, p)
    a.set_camera(None)
    after = run(a)
    a.close()
    b = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=4)
    fresh = run(b)
    b.close()
    assert before == after == fresh
    assert np.asarray(with_cam[5]).tobytes() != before[5]      # (the camera did change the association)


# ---- 6. the combiner is bypassed -------------------------------------------------------------------------------------------------
def test_camera_context_bypasses_the_combiner(oracle, oracle_euroc, euroc_l, euroc_r):
    import gf_orb_slam2_amd as G
    kl, dl, kr, dr, sf = oracle_euroc
    p = _params()
    e = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=2, combining=True)
    try:
        e.set_camera(*LEFT, right=RIGHT)
        got = e.extract_stereo_un(euroc_l, euroc_r, p)
        kp, ku, _ = e.extract_un(euroc_l)
        assert e.combiner_stats() == (0, 0), "a context with a camera must take the direct path"
        ul, ur = U.undistort_stereo(kl, kr, LEFT, RIGHT)
        _bits_equal(got[1], ul, "mvKeysUn")
        _bits_equal(got[4], ur, "mvKeysRightUn")
        _cmp_stereo(got[6:], oracle.stereo_match(ul, dl, ur, dr, sf, p.n_rows, p.mbf, p.mb, p.min_x))
        _bits_equal(ku, U.undistort_keypoints(kl, *LEFT), "extract_un, left camera")
    finally:
        e.close()


# ---- 7. malformed cameras ---------------------------------------------------------------------------------------------------------
def _bad_cameras():
    from gf_orb_slam2_amd._lib import make_camera
    out = []
    c = make_camera(U.K_L, U.D_L); c.K[0] = 0.0; out.append(("fx = 0", c))
    c = make_camera(U.K_L, U.D_L); c.K[4] = 0.0; out.append(("fy = 0", c))
    c = make_camera(U.K_L, U.D_L); c.D[1] = float("nan"); out.append(("NaN coefficient", c))
    c = make_camera(U.K_L, U.D_L, U.R_L, U.P_L); c.R[4] = float("inf"); out.append(("inf in R", c))
    c = make_camera(U.K_L, U.D_L, U.R_L, U.P_L); c.P[11] = float("nan"); out.append(("NaN in P", c))
    c = make_camera(U.K_L, U.D_L); c.K[2] = float("inf"); out.append(("inf in K", c))
    for n in (0, 3, 6, 12, 14, -1):
        c = make_camera(U.K_L, U.D_L); c.n_dist = n; out.append((f"n_dist {n}", c))
    c = make_camera(U.K_L, U.D_L); c.has_R = 2; out.append(("has_R 2", c))
    return out


def test_malformed_cameras_are_refused(ext, oracle, oracle_euroc, euroc_l, euroc_r):
    from gf_orb_slam2_amd._lib import make_camera
    L = ext._L
    kl, dl, kr, dr, sf = oracle_euroc
    good_l, good_r = make_camera(*LEFT), make_camera(*RIGHT)
    assert L.gfo_ctx_set_camera(ext.handle, C.byref(good_l), C.byref(good_r)) == 0
    xy = _dense_points()
    for name, bad in _bad_cameras():
        for args in ((C.byref(bad), None), (C.byref(good_l), C.byref(bad)), (C.byref(bad), C.byref(good_r))):
            assert L.gfo_ctx_set_camera(ext.handle, *args) == -1, name
        out = np.full_like(xy, 7.0)
        assert L.gfo_undistort_points(ext.handle, C.byref(bad), xy.ctypes.data_as(C.c_void_p), len(xy), out.ctypes.data_as(C.c_void_p)) == -1, name
        assert (out == 7.0).all(), f"{name}: outputs touched"
    assert L.gfo_ctx_set_camera(ext.handle, None, C.byref(good_r)) == -1          # a right camera without a left one
    # the context kept the rig: the next call equals the oracle
    p = _params()
    got = ext.extract_stereo_un(euroc_l, euroc_r, p)
    ul, ur = U.undistort_stereo(kl, kr, LEFT, RIGHT)
    _bits_equal(got[1], ul, "mvKeysUn after refused calls")
    _cmp_stereo(got[6:], oracle.stereo_match(ul, dl, ur, dr, sf, p.n_rows, p.mbf, p.mb, p.min_x))
    # a refused extraction argument leaves the caller's arrays alone too
    n = C.c_int(-5)
    assert L.gfo_extract_un(ext.handle, euroc_l.ctypes.data_as(C.c_void_p), 752, 480, 752, None, None, None, 4, C.byref(n)) == -1
    assert n.value == -5
    # setting the same cameras again is a no-op: the last batch stays fetchable
    assert L.gfo_ctx_set_camera(ext.handle, C.byref(good_l), C.byref(good_r)) == 0
    _bits_equal(ext.batch_fetch_un(0), ul, "after re-setting the same rig")


# ---- the captured launch sequence (GFO_GRAPH=1) --------------------------------------------------------------------------------------
def test_graph_replay_returns_this_calls_undistorted_keypoints(oracle, oracle_euroc, euroc_l, euroc_r, monkeypatch):
    """with the launch sequence captured as a hipGraph, a per-frame call that returns the undistorted arrays must not replay the graph
    of a call that did not (its result pack has two more segments), nor the other way round"""
    import gf_orb_slam2_amd as G
    monkeypatch.setenv("GFO_GRAPH", "1")
    kl, dl, kr, dr, sf = oracle_euroc
    ul, ur = U.undistort_stereo(kl, kr, LEFT, RIGHT)
    p = _params()
    ref = oracle.stereo_match(ul, dl, ur, dr, sf, p.n_rows, p.mbf, p.mb, p.min_x)
    e = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=2)
    try:
        e.set_camera(*LEFT, right=RIGHT)
        for _ in range(2):
            _cmp_stereo(e.extract_stereo(euroc_l, euroc_r, p)[4:], ref)
            got = e.extract_stereo_un(euroc_l, euroc_r, p)
            _bits_equal(got[1], ul, "mvKeysUn after a plain stereo call")
            _bits_equal(got[4], ur, "mvKeysRightUn after a plain stereo call")
            _cmp_stereo(got[6:], ref)
        # one image: gfo_extract, then gfo_extract_un, on a mono camera
        e.set_camera(U.K_L, U.D_L)
        want = U.undistort_mono(kl, U.K_L, U.D_L)
        for _ in range(2):
            assert e(euroc_l)[0].tobytes() == kl.tobytes()
            kp, ku, _ = e.extract_un(euroc_l)
            assert kp.tobytes() == kl.tobytes()
            _bits_equal(ku, want, "mvKeysUn after a plain extraction")
    finally:
        e.close()


def test_set_camera_requires_the_coefficients(ext):
    with pytest.raises(ValueError, match="distortion coefficients"):
        ext.set_camera(U.K_L)
