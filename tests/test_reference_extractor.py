"""The oracle's extractor against the REFERENCE's own src/ORBextractor.cc, compiled unmodified (oracle/_ref/libref_orbextractor*.so,
oracle/Makefile `ref`) with OpenCV's arithmetic routed to the oracle's [OCV] primitives (oracle/ref_shim/cv_arith.h).  Everything
but FAST / resize / GaussianBlur / fastAtan2 / cvRound is then the reference's compiled code: the constructor tables, ComputePyramid's
frame, the cell grid and its threshold fallback, DistributeOctTree, IC_Angle, computeOrbDescriptor and operator()'s level layout.
Bit for bit: floats by bit pattern, keypoint arrays by bytes.  Each build is compared with the oracle variant that states its
arithmetic (orb_oracle.REF_EXTRACTOR_BUILDS): -ffp-contract=off with (TRIG_LIBM, ROT_UNFUSED), the reference's own -O3 (contracted)
with (TRIG_LIBM, ROT_FMA).

Skip rule as test_oracle.py::test_bow_fold_against_the_reference_build_live: only where neither the libraries nor the reference tree
exist.  Where the tree exists a missing or stale library is a failure."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, synth_frame, load_u8
from test_gpu_fuzz import _random_image

REF_SRC = os.path.join("src", "ORBextractor.cc")


@pytest.fixture(scope="module")
def ref(oracle):
    """the RefExtractor class, once both builds are known to exist and to be current"""
    tree = os.path.exists(os.path.join(oracle.REFERENCE_ROOT, REF_SRC))
    have = [os.path.exists(oracle.ref_extractor_path(b)) for b in oracle.REF_EXTRACTOR_BUILDS]
    if not tree and not all(have):
        pytest.skip("oracle/_ref/libref_orbextractor*.so not built (no reference tree on this machine)")
    for b, ok in zip(oracle.REF_EXTRACTOR_BUILDS, have):
        assert ok, f"{oracle.ref_extractor_path(b)} is missing: __graft_entry__.build() (make -C oracle ref) makes it"
        stale = oracle.ref_extractor_stale(b)
        assert not stale, f"{oracle.ref_extractor_path(b)} is older than {stale}: rebuild with make -C oracle ref"
    return oracle.RefExtractor


def _f32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(R, oracle, img, nf=1000, sf=1.2, nl=8, ini=20, mn=7, build="unfused"):
    """the reference build and its matching oracle variant on one image: keypoints by bytes, descriptors by value"""
    r = R(nf, sf, nl, ini, mn, build=build)
    kr, dr = r(img)
    o = r.oracle()
    ko, do = o(img)
    assert kr.tobytes() == ko.tobytes(), f"keypoints differ ({build}, {img.shape}, nf={nf} sf={sf} nl={nl} th={ini}/{mn})"
    assert dr.shape == do.shape and (dr == do).all(), f"descriptors differ ({build}, {img.shape})"
    return len(kr)


def test_descriptors_are_written_through_the_row_views(ref, oracle, euroc_l):
    """computeDescriptors (ORBextractor.cc:1105) assigns Mat::zeros to a rowRange view of the output: the stand-in must fill the
    view in place, as OpenCV's MatExpr does.  Rebinding the view would hand back the output as create() left it (zeros)."""
    kr, dr = ref(2000, 1.2, 8, 20, 7)(euroc_l)
    assert len(kr) > 1500
    assert (dr.any(axis=1)).all(), "a descriptor row came back all zero"
    o = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    o.set_variant(oracle.TRIG_LIBM, oracle.ROT_UNFUSED)
    assert (o(euroc_l)[1] == dr).all()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_standin_zeros_fills_a_view_in_place(tmp_path):
    """the stand-in's Mat::zeros semantics on their own: assigned to a view of the same size and type it zero-fills the parent's
    rows; a Mat constructed from it is a new allocation"""
    src = tmp_path / "z.cc"
    src.write_text(r'''
#include <opencv/cv.h>
int main() {
    cv::Mat m(4, 8, CV_8UC1, cv::Scalar(7));
    cv::Mat v = m.rowRange(1, 3);
    cv::Mat& r = v;
    r = cv::Mat::zeros(2, 8, CV_8UC1);
    if (v.data != m.data + m.step) return 1;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 8; j++) if (m.at<unsigned char>(i, j) != ((i == 1 || i == 2) ? 0 : 7)) return 2;
    cv::Mat n = cv::Mat::zeros(3, 5, CV_8UC1);
    if (n.rows != 3 || n.cols != 5 || n.data == m.data || n.at<unsigned char>(2, 4) != 0) return 3;
    return 0;
}
''')
    exe = tmp_path / "z"
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "tests", "cv_standin"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


@pytest.mark.parametrize("nf,sf,nl,ini,mn", [(500, 1.2, 8, 20, 7), (3000, 1.1, 12, 12, 5), (50, 1.5, 4, 40, 10), (1000, 2.0, 3, 20, 7),
                                             (1200, 1.2, 1, 20, 7), (7, 1.2, 8, 20, 7), (4000, 1.2, 8, 20, 7), (6000, 1.2, 2, 20, 7),
                                             (6000, 1.2, 3, 20, 7), (7, 1.4, 3, 20, 7), (7, 1.05, 20, 20, 7)])
def test_constructor_tables(ref, oracle, nf, sf, nl, ini, mn):
    """ORBextractor::ORBextractor (:409-469): scale factors, sigma^2 and inverses, features per level, umax, the pattern"""
    t = ref(nf, sf, nl, ini, mn).tables()
    o = oracle.OracleExtractor(nf, sf, nl, ini, mn)
    for k in ("scale_factors", "inv_scale_factors", "level_sigma2", "inv_level_sigma2"):
        np.testing.assert_array_equal(_f32(t[k]), _f32(getattr(o, k)), err_msg=k)
    np.testing.assert_array_equal(t["features_per_level"], o.features_per_level)
    np.testing.assert_array_equal(t["umax"], o.umax)
    text = open(os.path.join(ROOT, "include", "gfo_pattern.inc")).read()
    body = text[text.index("*/") + 2:]
    pairs = np.array([int(x) for x in body.replace("{", " ").replace("}", " ").replace(",", " ").split()], np.int32).reshape(512, 2)
    np.testing.assert_array_equal(t["pattern"], pairs)      # the kernels' pattern = the reference's bit_pattern_31_


@pytest.mark.parametrize("side", ["l", "r"])
def test_golden_files(ref, oracle, side):
    """tests/golden/EuRoC_*: made by the oracle with its default, correctly rounded sin / cos.  The reference build reproduces the
    keypoints and the per-level counts; a descriptor row may differ only where the oracle's TRIG_LIBM and TRIG_SHARED runs differ."""
    img = load_u8(f"EuRoC_{side}_752x480.u8")
    gk = np.fromfile(os.path.join(GOLDEN, f"EuRoC_{side}_kp.bin"), oracle.KEYPOINT_DTYPE)
    gd = np.fromfile(os.path.join(GOLDEN, f"EuRoC_{side}_desc.bin"), np.uint8).reshape(-1, 32)
    lv = np.load(os.path.join(GOLDEN, f"EuRoC_{side}_levels.npz"))
    r = ref(2000, 1.2, 8, 20, 7)
    kr, dr = r(img)
    assert kr.tobytes() == gk.tobytes()
    calls, _ = r.fast_log()
    sizes = [r.level_size(l) for l in range(8)]
    for l in range(8):
        mine = calls[(calls["level_w"] == sizes[l][0]) & (calls["level_h"] == sizes[l][1])]
        assert mine["count"].sum() == lv["ncand"][l], l
        assert (kr["octave"] == l).sum() == lv["per_level"][l], l
    o = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    o.set_variant(oracle.TRIG_LIBM, oracle.ROT_UNFUSED)
    assert (o(img)[1] == dr).all()
    trig_rows = set(np.nonzero((o(img)[1] != gd).any(axis=1))[0])
    diff = set(np.nonzero((dr != gd).any(axis=1))[0])
    assert diff <= trig_rows, sorted(diff - trig_rows)[:10]


# the sizes of test_gpu_sizes.py::test_awkward_sizes_one_context, odd widths, and images so small that the top levels hold no cell
PYR_SIZES = [(1241, 376), (333, 217), (130, 100), (64, 48), (37, 300), (753, 481), (641, 479), (1001, 5), (39, 41), (23, 17), (6, 5)]


@pytest.mark.parametrize("w,h", PYR_SIZES)
@pytest.mark.parametrize("sf,nl", [(1.2, 8), (1.4, 6), (2.0, 4)])
def test_pyramid_levels(ref, oracle, w, h, sf, nl):
    """ComputePyramid (:1176-1201): every level, without and with the 19-px BORDER_REFLECT_101 frame the reference writes"""
    img = synth_frame(w, h, 3 * w + h) if min(w, h) >= 8 else np.random.default_rng(w).integers(0, 256, (h, w), dtype=np.uint8)
    r = ref(1000, sf, nl, 20, 7)
    r.compute_pyramid(img)
    o = oracle.OracleExtractor(1000, sf, nl, 20, 7)
    o.compute_pyramid(img)
    for l in range(nl):
        assert r.level_size(l) == o.level_size(l), l
        np.testing.assert_array_equal(r.level(l), o.level(l), err_msg=f"level {l}")
        np.testing.assert_array_equal(r.level(l, padded=True), o.level(l, padded=True), err_msg=f"padded level {l}")


def test_a_level_that_rounds_to_nothing(ref, oracle):
    """A 1-px wide image: level 4 rounds to no column.  cv::resize asserts there (the reference does not catch it); the oracle keeps
    the empty level and reads nothing through it."""
    img = np.arange(5, dtype=np.uint8).reshape(5, 1)
    r = ref(100, 1.2, 8, 20, 7)
    with pytest.raises(oracle.RefExtractorError):
        r.compute_pyramid(img)
    o = oracle.OracleExtractor(100, 1.2, 8, 20, 7)
    o.compute_pyramid(img)
    assert [o.level_size(l)[0] for l in range(8)] == [1, 1, 1, 1, 0, 0, 0, 0]


def _log_by_level(r, nl):
    calls, corners = r.fast_log()
    out = []
    for l in range(nl):
        w, h = r.level_size(l)
        out.append((calls[(calls["level_w"] == w) & (calls["level_h"] == h)], corners))
    return out


@pytest.mark.parametrize("ini,mn", [(1, 1), (7, 2), (20, 7)])
@pytest.mark.parametrize("kind", [1, 2])
def test_fast_log_against_level_candidates(ref, oracle, ini, mn, kind):
    """Every cv::FAST call of ComputeKeyPointsOctTree (:796-839), level by level, against OracleExtractor.level_candidates: the ROI of
    each cell, the iniThFAST call and the minThFAST call that follows it exactly when the first found nothing, and the corners
    with the cell offsets (:825-826) added -- in the order DistributeOctTree receives them."""
    rng = np.random.default_rng(ini * 10 + kind)
    img = _random_image(rng, 640, 480, kind)
    r = ref(1500, 1.2, 8, ini, mn)
    kr, _ = r(img)
    o = oracle.OracleExtractor(1500, 1.2, 8, ini, mn)
    o(img)
    fallbacks = 0
    for l, (calls, corners) in enumerate(_log_by_level(r, 8)):
        got = []
        k = 0
        while k < len(calls):
            c = calls[k]
            assert c["threshold"] == ini, (l, k)
            if c["count"] == 0:           # :813-817: the same cell again at minThFAST
                nx = calls[k + 1]
                assert nx["threshold"] == mn and [nx[f] for f in "xywh"] == [c[f] for f in "xywh"], (l, k)
                fallbacks += 1
                k += 1
                c = nx
            xy = corners[c["first"]:c["first"] + c["count"]].copy()
            xy[:, 0] += c["x"] - 16       # minBorderX + j * wCell, less minBorderX
            xy[:, 1] += c["y"] - 16
            got.append(xy)
            k += 1
        got = np.concatenate(got) if got else np.zeros((0, 3), np.int32)
        np.testing.assert_array_equal(got, o.level_candidates(l), err_msg=f"level {l}")
        assert (kr["octave"] == l).sum() == o.level_keypoint_count(l), l
    if kind == 2 and ini > 1:
        assert fallbacks > 0      # low-contrast noise reaches the minThFAST pass


KINDS = 5


def test_fuzz_slice(ref, oracle):
    """A seeded slice of the fuzz corpus (test_gpu_fuzz.py's five image kinds, its size / nf / scale / level ranges, random
    thresholds), alternating the two builds: at least 100 completed cases.  A draw the reference cannot complete -- a node count that
    rounds below one on some level: it throws (negative) or would index an empty vector (zero) -- is counted, not compared."""
    rng = np.random.default_rng(2024)
    done, refused, kinds = 0, 0, set()
    for it in range(400):
        w, h = int(rng.integers(64, 1000)), int(rng.integers(48, 700))
        nf = int(rng.choice([50, 300, 1000, 2000]))
        sf = float(rng.choice([1.1, 1.2, 1.2, 1.3, 1.5, 2.0]))
        nl = int(rng.integers(2, 11 if sf < 1.4 else 5))
        ini = int(rng.choice([20, 20, 12, 40, 5]))
        mn = int(rng.choice([7, 7, 3, 1, ini]))
        kind = it % KINDS
        img = _random_image(rng, w, h, kind)
        try:
            _same(ref, oracle, img, nf, sf, nl, ini, mn, build=("unfused", "fma")[it % 2])
        except oracle.RefExtractorError:
            refused += 1
            continue
        done += 1
        kinds.add(kind)
        if done == 110:
            break
    assert done == 110 and kinds == set(range(KINDS)), (done, refused)


@pytest.mark.parametrize("build", ["unfused", "fma"])
def test_large_images(ref, oracle, build):
    """1920x1080 @ 4000 and the 4000x3000 tile of test_maximum_image_size @ 5000"""
    assert _same(ref, oracle, synth_frame(1920, 1080, 5), 4000, build=build) > 3000
    base = synth_frame(1000, 750, 99)
    assert _same(ref, oracle, np.ascontiguousarray(np.tile(base, (4, 4))), 5000, build=build) >= 4000


@pytest.mark.parametrize("nf,nl,w,h", [(4000, 1, 752, 480), (6000, 2, 1241, 376), (6000, 3, 640, 480)])
def test_level_quotas_above_2040(ref, oracle, nf, nl, w, h):
    """the quotas of test_large_level_quota_runs_from_global_memory: DistributeOctTree with more than 2040 nodes wanted"""
    assert oracle.OracleExtractor(nf, 1.2, nl, 20, 7).features_per_level.max() > 2040
    assert _same(ref, oracle, synth_frame(w, h, nf + nl), nf, 1.2, nl) > 500
    assert _same(ref, oracle, synth_frame(w, h, 77), nf, 1.2, nl, build="fma") > 500


def test_flat_faint_saturated_and_empty(ref, oracle):
    assert _same(ref, oracle, np.full((480, 752), 128, np.uint8)) == 0
    faint = (128 + 6 * ((np.indices((480, 752)).sum(0) // 23) % 2)).astype(np.uint8)      # contrast 12 < iniTh
    faint[::37, ::41] += 9
    assert _same(ref, oracle, faint) > 0
    blocks = np.where((np.indices((480, 752)) // 16).sum(0) % 2 == 0, 255, 0).astype(np.uint8)
    _same(ref, oracle, blocks)
    _same(ref, oracle, np.full((480, 752), 255, np.uint8))
    kr, dr = ref(1000, 1.2, 8, 20, 7)(np.zeros((0, 0), np.uint8))      # :1115: an empty image returns at once
    assert len(kr) == 0 and len(dr) == 0


def test_ocv_switches_reach_the_reference_build(ref, oracle, euroc_l):
    """One non-default [OCV] set on both sides: the reference build calls the same loaded oracle, so it follows the switches --
    and what it computes under them changes."""
    img = euroc_l[60:420, 100:660]
    before = ref(1000, 1.2, 8, 20, 7)(img)
    saved = oracle.get_ocv_variants()
    try:
        oracle.set_ocv_variants(resize=1, atan_fma=1, blur_round=1)
        after = ref(1000, 1.2, 8, 20, 7)(img)
        assert after[0].tobytes() != before[0].tobytes()
        _same(ref, oracle, img)
        _same(ref, oracle, img, build="fma")
    finally:
        oracle.set_ocv_variants(**saved)


def test_the_arena_serves_the_reference_list_nodes(ref, oracle, euroc_l):
    """The bump arena (orbextractor_shim.cc) served every allocation of the call, the std::list<ExtractorNode> nodes of
    DistributeOctTree among them; with the system allocator switched on malloc serves them instead."""
    r = ref(2000, 1.2, 8, 20, 7)
    r(euroc_l)
    st = r.arena_stats()
    assert st["list_nodes"] > 1000 and st["arena"] >= st["list_nodes"] and st["malloc"] == 0 and st["overflows"] == 0
    oracle.ref_set_system_allocator(True)
    try:
        r(euroc_l)
        st = r.arena_stats()
        assert st["arena"] == 0 and st["malloc"] >= st["list_nodes"] > 1000
    finally:
        oracle.ref_set_system_allocator(False)
