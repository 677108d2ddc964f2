"""The vertical blend of the batch-path pyramid kernels (k_pyramid.hip rs_blend) against resize_vblend's expression and
the oracle's VResizeLinear statement, over every row coefficient b in 0..2048 and every horizontal sum h in 0..255*2048
the kernels can meet.  rs_blend takes each row's h >> 4 once and forms (b * x) >> 16 as the high word of (b << 16) * x;
the >> 2 of the rounded sum runs on two 16-bit halves at once.  No GPU needed."""
import numpy as np

B_MAX = 2048            # 11-bit coefficients: lrintf(f * 2048) for f in [0, 1]
H_MAX = 255 * 2048      # a horizontal sum: two bytes times coefficients that add to 2048


def _v1(b0, b1, ha, hb):
    """resize_vblend (GFO_OCV_RESIZE 0): __umul24 on the shifted sums, >> 16 each, + 2, >> 2, & 255"""
    return ((((b0 * (ha >> 4)) & 0xFFFFFFFF) >> 16) + (((b1 * (hb >> 4)) & 0xFFFFFFFF) >> 16) + 2) >> 2 & 255


def _oracle(b0, b1, ha, hb):
    """VResizeLinear<uchar, int, short> with FixedPtCast<int, uchar, 2>: (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16)
    + 2) >> 2, saturated to uchar"""
    v = (((b0 * (ha >> 4)) >> 16) + ((b1 * (hb >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255)


def _mul_hi(a, b):
    return (a.astype(np.uint64) * b.astype(np.uint64) >> np.uint64(32)).astype(np.int64)


def _v2(b0, b1, xa, xb):
    """rs_blend on one byte: x = h >> 4 taken by rs_hsum; mul_hi(b0 << 16, xa) + mul_hi(b1 << 16, xb) + 2; the >> 2 as
    v_pk_lshrrev_b16 does it on the 16-bit half the sum sits in, and v_perm_b32 keeps the low byte of each half"""
    s = _mul_hi((b0 << 16) & 0xFFFFFFFF, xa) + _mul_hi((b1 << 16) & 0xFFFFFFFF, xb) + 2
    assert (s < 1 << 16).all()
    return ((s & 0xFFFF) >> 2) & 255


def test_mul_hi_identity_full_range():
    """(b * x) >> 16 == mul_hi(b << 16, x) for every b in 0..2048 and x in 0..H_MAX >> 4 (exhaustive in x, b in blocks)"""
    x = np.arange(0, (H_MAX >> 4) + 1, dtype=np.int64)
    for b in range(0, B_MAX + 1):
        bb = np.full_like(x, b)
        np.testing.assert_array_equal(_mul_hi(bb << 16, x), (bb * x) >> 16, err_msg=f"b={b}")


def test_blend_equals_old_and_oracle():
    rng = np.random.default_rng(11)
    n = 4_000_000
    b0 = rng.integers(0, B_MAX + 1, n)
    b1 = np.where(rng.random(n) < 0.5, B_MAX - b0, rng.integers(0, B_MAX + 1, n))   # pairs that add to 2048, and any pair
    ha = rng.integers(0, H_MAX + 1, n)
    hb = rng.integers(0, H_MAX + 1, n)
    # the corners: zero and full coefficients, zero and saturated sums
    corners = np.array(np.meshgrid([0, 1, 1024, 2047, 2048], [0, 1, 1024, 2047, 2048], [0, 15, 16, H_MAX - 1, H_MAX],
                                   [0, 15, 16, H_MAX - 1, H_MAX])).reshape(4, -1)
    b0, b1, ha, hb = (np.concatenate([v, c]) for v, c in zip((b0, b1, ha, hb), corners))
    sum_ok = b0 + b1 <= B_MAX
    new = _v2(b0, b1, ha >> 4, hb >> 4)
    np.testing.assert_array_equal(new, _v1(b0, b1, ha, hb))
    # the oracle saturates; with b0 + b1 <= 2048 (every table the plan builds) the sum never needs it
    np.testing.assert_array_equal(new[sum_ok], _oracle(b0, b1, ha, hb)[sum_ok])
    assert (new[sum_ok] == ((_mul_hi(b0 << 16, ha >> 4) + _mul_hi(b1 << 16, hb >> 4) + 2) >> 2)[sum_ok]).all()   # no byte lost


def test_blend_exhaustive_in_h_for_table_coefficients():
    """Every coefficient pair b0 + b1 = 2048 a row table holds, against every x = h >> 4 of one row with the other row
    at its extremes and midpoint."""
    x = np.arange(0, (H_MAX >> 4) + 1, dtype=np.int64)
    for b0 in range(0, B_MAX + 1, 7):
        b1 = B_MAX - b0
        for xb in (0, 1, (H_MAX >> 4) // 2, H_MAX >> 4):
            xbv = np.full_like(x, xb)
            new = _v2(np.full_like(x, b0), np.full_like(x, b1), x, xbv)
            np.testing.assert_array_equal(new, _v1(np.full_like(x, b0), np.full_like(x, b1), x << 4, xbv << 4))
