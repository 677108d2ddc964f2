"""The stereo association without a camera, on host arrays whose right keypoints lie above the image: a right keypoint whose row
band [floor(y - r), ceil(y + r)] misses the rows enters no row of PrepareStereoCandidates (Frame.cc:1167-1176: the loop over its rows
does not run).  k_stereo_bucket packs such a band as an empty one; the row form's staged (first row, height) record once read the old
empty band (1, 0) as "every row", and left keypoints near the top then matched keypoints the reference never offers them.  Every form
of the association against orb_oracle.stereo_match, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FX, BF = 435.2046959714599, 47.90639384423901


@pytest.fixture(scope="module")
def shifted(oracle, euroc_l, euroc_r):
    """the EuRoC pair's oracle keypoints moved 80 rows up (left keypoints in the top rows, right ones above the image), plus one decoy
    per left keypoint of the top rows: a right keypoint with the SAME descriptor, the same octave and a disparity of 5 px, placed just
    above the image so that its band misses it -- the reference never offers it, an association that does takes it (distance 0)"""
    oe = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    kl, dl = oe(euroc_l)
    kr, dr = oe(euroc_r)
    sf = oe.scale_factors
    kl, kr = kl.copy(), kr.copy()
    kl["y"] -= np.float32(80.0)
    kr["y"] -= np.float32(80.0)
    top = np.nonzero((kl["y"] >= 0) & (kl["y"] < 8))[0]
    decoy = kl[top].copy()
    decoy["x"] = kl["x"][top] - np.float32(5.0)
    decoy["y"] = -(2.0 * sf[kl["octave"][top]]).astype(np.float32) - np.float32(1.5)
    return kl, dl, np.concatenate([kr, decoy]), np.concatenate([dr, dl[top]]), sf


@pytest.mark.parametrize("form", ["default", "rows", "keypoints"])
def test_right_keypoints_whose_band_misses_the_image(oracle, shifted, form, monkeypatch):
    import gf_orb_slam2_amd as G
    if form == "rows":
        monkeypatch.setenv("GFO_STEREO_ROWS", "5")
    elif form == "keypoints":
        monkeypatch.setenv("GFO_STEREO_ROWS", "0")
    kl, dl, kr, dr, sf = shifted
    rr = 2.0 * sf[kr["octave"]]
    assert (np.ceil(kr["y"] + rr) < 0).sum() > 20           # bands that miss the image
    assert ((kl["y"] >= 0) & (kl["y"] < 8)).sum() > 20       # left keypoints whose search window reaches row 0
    ext = G.ORBextractor(2000, 1.2, 8, 20, 7)
    try:
        m = G.ORBmatcher(0.8, True, extractor=ext)
        p = G.StereoParams(480, BF, BF / FX, 0.0)
        got = m.ComputeStereoMatches(kl, dl, kr, dr, sf, p)
    finally:
        ext.close()
    ref = oracle.stereo_match(kl, dl, kr, dr, sf, p.n_rows, p.mbf, p.mb, p.min_x)
    assert got[0] == ref[0], f"nmatched {got[0]} vs {ref[0]}"
    for name, a, b in zip(("u_right", "depth", "best_dist", "best_idx"), got[1:], ref[1:]):
        assert a.tobytes() == b.tobytes(), name
