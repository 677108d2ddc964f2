"""Every pyramid level of the batch path (k_resize for the big levels, k_resize_tail for the small top ones, the path
batches of 32 images and more take) against the oracle's ComputePyramid, image by image: batch sizes 32, 33 and 256,
widths 752, 753 (odd rows), 640 and 1920, and scale factors above 1.33 (rows of a strip that advance by two source rows).
Bit-exact."""
import numpy as np
import pytest

from conftest import synth_frame

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,nimg,sf,nl", [
    (752, 480, 32, 1.2, 8),
    (753, 480, 33, 1.2, 8),
    (752, 480, 256, 1.2, 8),
    (640, 480, 33, 1.2, 8),
    (1920, 1080, 32, 1.2, 8),
    (753, 481, 33, 1.4, 6),
    (752, 480, 32, 1.6, 5),
    (641, 479, 33, 2.0, 4),
])
def test_batch_pyramid_every_level(oracle, monkeypatch, w, h, nimg, sf, nl):
    import gf_orb_slam2_amd as G
    monkeypatch.setenv("GFO_PYR_BAND_MIN_WG", "100000000")   # the per-level kernels even where a batch could take the bands
    imgs = [synth_frame(w, h, 13 * w + i) for i in range(3)]
    batch = [imgs[i % len(imgs)] for i in range(nimg)]
    ext = G.ORBextractor(1000, sf, nl, 20, 7, max_batch=nimg)
    oe = oracle.OracleExtractor(1000, sf, nl, 20, 7)
    ext.extract_batch(batch)
    for i in sorted({0, 1, 2, nimg - 1}):
        oe.compute_pyramid(batch[i])
        for l in range(nl):
            np.testing.assert_array_equal(ext.pyramid_level(l, image=i), oe.level(l), err_msg=f"image {i} level {l}")
    ext.close()
