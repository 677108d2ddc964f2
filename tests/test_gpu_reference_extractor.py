"""The kernels against the REFERENCE's own ORBextractor.cc (oracle/_ref/libref_orbextractor.so: the file compiled unmodified,
-ffp-contract=off, OpenCV's arithmetic routed to the oracle's [OCV] primitives; tests/test_reference_extractor.py pins the oracle to
it on the CPU).  The library is the one __graft_entry__.build() left in oracle/_ref/; the reference tree is never read here.

Pyramid levels (with their 19-px frame), keypoints and angles: bit for bit.  Descriptors: bit for bit, except rows where the
reference build's libm cosf / sinf and the kernels' correctly rounded gfo_sincos give different bits -- each such row must be one
where the oracle's TRIG_LIBM and TRIG_SHARED runs differ too.  How many rows that is, is printed per case."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, synth_frame

pytestmark = pytest.mark.gpu

STEREO_BF, STEREO_FX = 47.90639384423901, 435.2046959714599


@pytest.fixture(scope="module")
def ref(oracle):
    path = oracle.ref_extractor_path("unfused")
    if not os.path.exists(path):
        if os.path.exists("/root/reference/include/ORBextractor.h"):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
        else:
            # (a skip, not a failure, as in test_gpu_adapter_run.py: the library goes with oracle/_ref/ from where build() made it)
            pytest.skip("oracle/_ref/libref_orbextractor.so is missing and the reference tree is not here: "
                        "__graft_entry__.build() makes the library where it is and it goes with oracle/_ref/")
    return oracle.RefExtractor


def _check(oracle, r, img, kp, desc, label):
    """kernel output (kp, desc) of one image against the reference build r, which has just run on img"""
    kr, dr = r(img)
    assert len(kp) == len(kr), f"{label}: {len(kp)} keypoints, the reference {len(kr)}"
    assert kp.tobytes() == kr.tobytes(), f"{label}: keypoints (angles included) differ from the reference build"
    rows = np.nonzero((desc != dr).any(axis=1))[0]
    if len(rows):
        libm = r.oracle()
        shared = oracle.OracleExtractor(r.nfeatures, r._scale_factor_arg, r.nlevels, r._ini, r._min)
        shared.set_variant(oracle.TRIG_SHARED, oracle.ROT_UNFUSED)
        trig = (libm(img)[1] != shared(img)[1]).any(axis=1)
        assert trig[rows].all(), f"{label}: descriptor rows {rows[~trig[rows]][:10]} differ from the reference, not by the trig choice"
    print(f"\n[trig rows] {label}: {len(rows)} of {len(kp)} descriptor rows differ by libm cosf/sinf vs gfo_sincos")
    return len(kp)


def _check_levels(ext, r, img, nl, image=0):
    r.compute_pyramid(img)
    for l in range(nl):
        np.testing.assert_array_equal(ext.pyramid_level(l, image=image, border=19), r.level(l, padded=True), err_msg=f"level {l}")


@pytest.mark.parametrize("side", ["l", "r"])
def test_euroc_single_and_batched(ref, oracle, euroc_l, euroc_r, side):
    import gf_orb_slam2_amd as G
    img = euroc_l if side == "l" else euroc_r
    other = euroc_r if side == "l" else euroc_l
    ext = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=4)
    r = ref(2000, 1.2, 8, 20, 7)
    kp, desc = ext(img)
    assert _check(oracle, r, img, kp, desc, f"EuRoC {side} single") > 1500
    _check_levels(ext, r, img, 8)
    kps, descs = ext.extract_batch([other, img, img[::-1].copy(), other])
    _check(oracle, r, img, kps[1], descs[1], f"EuRoC {side} batched")
    _check(oracle, r, img[::-1].copy(), kps[2], descs[2], f"EuRoC {side} flipped, batched")
    _check_levels(ext, r, img, 8, image=1)
    ext.close()


def test_batch_of_33_rolling_rows(ref, oracle, monkeypatch):
    """33 images of 753x481 at scale factor 1.4: the rolling-row pyramid kernels of the batch path (k_resize, k_resize_tail)"""
    import gf_orb_slam2_amd as G
    monkeypatch.setenv("GFO_PYR_BAND_MIN_WG", "100000000")
    imgs = [synth_frame(753, 481, 13 * 753 + i) for i in range(3)]
    batch = [imgs[i % 3] for i in range(33)]
    ext = G.ORBextractor(1000, 1.4, 6, 20, 7, max_batch=33)
    r = ref(1000, 1.4, 6, 20, 7)
    kps, descs = ext.extract_batch(batch)
    for i in (0, 1, 2, 32):
        _check(oracle, r, batch[i], kps[i], descs[i], f"753x481 sf 1.4 batch image {i}")
        _check_levels(ext, r, batch[i], 6, image=i)
    ext.close()


def test_1080p_at_4000(ref, oracle):
    import gf_orb_slam2_amd as G
    img = synth_frame(1920, 1080, 5)
    ext = G.ORBextractor(4000, 1.2, 8, 20, 7)
    r = ref(4000, 1.2, 8, 20, 7)
    kp, desc = ext(img)
    assert _check(oracle, r, img, kp, desc, "1920x1080 @ 4000") > 3000
    _check_levels(ext, r, img, 8)
    ext.close()


def test_level_quota_above_2040(ref, oracle):
    """6000 features on 2 levels: the global-memory quadtree (k_quadtree_gmem)"""
    import gf_orb_slam2_amd as G
    img = synth_frame(1241, 376, 6002)
    ext = G.ORBextractor(6000, 1.2, 2, 20, 7)
    assert ext.mnFeaturesPerLevel.max() > 2040
    r = ref(6000, 1.2, 2, 20, 7)
    kp, desc = ext(img)
    assert _check(oracle, r, img, kp, desc, "1241x376 @ 6000, 2 levels") > 500
    ext.close()


@pytest.mark.parametrize("w,h", [(1241, 376), (333, 217), (37, 300)])
def test_awkward_sizes(ref, oracle, w, h):
    import gf_orb_slam2_amd as G
    img = synth_frame(w, h, w + h)
    ext = G.ORBextractor(1000, 1.2, 8, 20, 7)
    r = ref(1000, 1.2, 8, 20, 7)
    kp, desc = ext(img)
    _check(oracle, r, img, kp, desc, f"{w}x{h}")
    _check_levels(ext, r, img, 8)
    ext.close()


def test_extract_stereo_left_and_right(ref, oracle, euroc_l, euroc_r):
    import gf_orb_slam2_amd as G
    ext = G.ORBextractor(2000, 1.2, 8, 20, 7)
    r = ref(2000, 1.2, 8, 20, 7)
    kl, dl, kr, dr, *_ = ext.extract_stereo(euroc_l, euroc_r, G.StereoParams(480, STEREO_BF, STEREO_BF / STEREO_FX, 0.0))
    _check(oracle, r, euroc_l, kl, dl, "extract_stereo left")
    _check(oracle, r, euroc_r, kr, dr, "extract_stereo right")
    ext.close()

