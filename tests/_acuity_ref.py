"""The yardstick of the receptor-noise-limited distance behind the observer's acuity blur (AcuityView, Caves & Johnsen 2018,
then Vorobyev & Osorio 1998) in NumPy float64 -- the definition of include/avx.h above avx_receptor_acuity_u8, no code under test.

Decode: lin = _deltae_ref.decode_table()[code].  Taps: k = cvRound(8 sigma + 1) | 1, t_i = exp(-(i - (k - 1) / 2)^2 / (2 sigma^2)) over
their sum added left to right (cv::getGaussianKernel), formed in float64.  Blur: every linear plane separably, rows (along x) first,
then columns; a sum runs over the taps in index order, s_0 = t_0 x_0, s_j = fma(t_j, x_j, s_(j-1)).  Border: BORDER_REFLECT_101 folded
as often as needed: p = 2 (n - 1), m = ((i mod p) + p) mod p, the index is m where m < n, else p - m; n = 1 gives 0.  Catches on the
blurred values in the anchored form, q_i = (g + R'_i0 (r - g)) + R'_i2 (b - g) with R' the matrix whose rows are divided by their sums
(_rnl_ref.catches' normalisation); the distance is _rnl_ref.delta_s_from_catches.  There is no "equal codes" rule.

dtype=np.float32 restates the same operations as a float32 device forms them: the table, the taps, R', the weights and the reciprocal
of the denominator are formed in float64 and rounded once, every operation on pixels is rounded to float32, and fma(t, x, s) is the
float64 product and sum rounded once to float32 (the product of two float32 is exact in float64).

frames(H, W) are the pairs the tests of both files (tests/test_acuity_host.py, tests/test_acuity_gpu.py) run on, CASES the sizes with
the sigmas each is run at, and BOUND the accuracy the device is held to: 8 x F32_FIGURE, the largest |float32 restatement - float64
yardstick| over all of them, which test_acuity_host.py measures and asserts."""
import math

import numpy as np

from _deltae_ref import CORNERS, decode_table
from _rnl_ref import delta_s_from_catches

MAX_KSIZE = 33
FOUR = [[0.7, 0.25, 0.05], [0.25, 0.65, 0.1], [0.05, 0.35, 0.6], [0.02, 0.12, 0.86]]  # test_receptor_gpu.py's four-class observer
KINDS = ("noise", "dark", "near", "ramp", "saturated", "spark")
# (H, W) -> the sigmas it is run at: every tap count (3, 7, 9, 29, 33) at the sizes every tap folds on, and at the larger sizes one small
# and one large radius, so that each seam of the 64 x 32 tile is crossed by a short and by a long halo; 96 x 160 is the smallest frame
# with a tile (the second of the second row) whose region lies inside the frame at the largest radius and so needs no folding
CASES = {(1, 1): (0.2, 0.7, 1.0, 3.5, 4.0), (2, 3): (0.2, 0.7, 1.0, 3.5, 4.0), (5, 7): (0.2, 0.7, 1.0, 3.5, 4.0), (16, 16): (1.0, 4.0),
         (33, 70): (0.7, 3.5), (48, 96): (0.2, 4.0), (70, 530): (1.0, 3.5, 4.0), (96, 160): (4.0,)}
# the largest |float32 restatement - float64 yardstick| over CASES x KINDS x the three observers, rounded up from the 2.35e-5 that
# test_acuity_host.py::test_float32_figure_that_sets_the_device_bound measures on a CPU (Dog, the ramp at 70 x 530, sigma 1.0; the
# four-class observer's largest is 1.65e-5, HoneyBee's 8.1e-6); the device's logf and division round differently from NumPy's, which
# is what the factor 8 is for (test_receptor_gpu.py's precedent)
F32_FIGURE = 2.5e-5
BOUND = 8 * F32_FIGURE
assert BOUND <= 1e-3


def ksize(sigma: float) -> int:
    """cvRound(8 sigma + 1) | 1: Python's round is cvRound (half to even)."""
    return int(round(sigma * 8 + 1)) | 1


def taps(sigma: float) -> np.ndarray:
    """cv::getGaussianKernel(ksize(sigma), sigma) in float64, the sum added left to right."""
    k = ksize(sigma)
    assert 3 <= k <= MAX_KSIZE
    c = (k - 1) * 0.5
    t = [math.exp(-0.5 / (sigma * sigma) * (i - c) * (i - c)) for i in range(k)]
    s = 0.0
    for v in t:
        s += v
    return np.array([v * (1.0 / s) for v in t], np.float64)


def fold(i, n: int):
    """BORDER_REFLECT_101 of index (array) i into 0 .. n - 1, folded as often as needed."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = ((i % p) + p) % p
    return np.where(m < n, m, p - m)


def _fma(t, x, s, dtype):
    if dtype is np.float64:
        return t * x + s
    return (np.float64(t) * x.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


def blur_axis(x: np.ndarray, t: np.ndarray, axis: int, dtype=np.float64) -> np.ndarray:
    """The sum over the taps along `axis`, in index order."""
    t = t.astype(dtype)
    n, R = x.shape[axis], (len(t) - 1) // 2
    at = np.arange(n)
    s = None
    for j in range(len(t)):
        xj = np.take(x, fold(at + j - R, n), axis=axis)
        s = t[j] * xj if s is None else _fma(t[j], xj, s, dtype)
        assert s.dtype == dtype
    return s


def blurred(rgb8: np.ndarray, sigma: float, dtype=np.float64) -> np.ndarray:
    """uint8 (..., H, W, 3) -> the blurred linear planes (..., H, W, 3): rows (along x) first, then columns."""
    lin = decode_table().astype(dtype)[np.asarray(rgb8)]
    t = taps(sigma)
    return blur_axis(blur_axis(lin, t, -2, dtype), t, -3, dtype)


def catches_of_linear(lin: np.ndarray, matrix, dtype=np.float64) -> np.ndarray:
    """Linear (..., 3) -> the catches (..., K) under the row-normalised matrix, in the anchored form."""
    m = np.asarray(matrix, np.float64)
    m = (m / m.sum(axis=1, keepdims=True)).astype(dtype)
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    dr, db = r - g, b - g
    q = np.stack([(g + m[i, 0] * dr) + m[i, 2] * db for i in range(len(m))], axis=-1)
    assert q.dtype == dtype
    return q


def delta_s(a, b, matrix, weber, floor, sigma, dtype=np.float64) -> np.ndarray:
    """uint8 (..., H, W, 3) pairs -> dS (..., H, W) behind the acuity blur of `sigma` pixels."""
    qa = catches_of_linear(blurred(a, sigma, dtype), matrix, dtype)
    qb = catches_of_linear(blurred(b, sigma, dtype), matrix, dtype)
    return delta_s_from_catches(qa, qb, weber, floor, dtype)


def near_mask(H: int, W: int, y: int, x: int, R: int) -> np.ndarray:
    """The pixels (H x W, bool) whose reflected (2R + 1)^2 neighbourhood holds pixel (y, x)."""
    d = np.arange(-R, R + 1)
    ys = (fold(np.arange(H)[:, None] + d[None, :], H) == y).any(axis=1)
    xs = (fold(np.arange(W)[:, None] + d[None, :], W) == x).any(axis=1)
    return ys[:, None] & xs[None, :]


# ------------------------------------------------------------------------------------------------ frames
_pairs = {}


def frames(H: int, W: int):
    """The six frame pairs of a size, in KINDS' order, as two stacks (6, H, W, 3); computed once, read-only.  The first five are
    test_receptor_gpu.py's: noise against other noise, a dark pair (codes // 16), a near-copy (+- 2 codes), a ramp against its
    channel-reversed self, saturated corners; the spark is black with one white pixel in A and one green pixel in B at the centre."""
    if (H, W) not in _pairs:
        rng = np.random.default_rng(H * 1000 + W)
        noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        other = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        near = np.clip(noise.astype(np.int16) + rng.integers(-2, 3, noise.shape), 0, 255).astype(np.uint8)
        y, x = np.mgrid[0:H, 0:W]
        ramp = np.stack([(255 * x) // max(1, W - 1), (255 * y) // max(1, H - 1), (255 * (x + y)) // max(1, H + W - 2)], axis=-1).astype(np.uint8)
        i = np.arange(H * W)
        ca, cb = CORNERS[(i // 8) % 8].reshape(H, W, 3), CORNERS[i % 8].reshape(H, W, 3)
        sa, sb = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
        sa[H // 2, W // 2] = 255
        sb[H // 2, W // 2] = (0, 255, 0)
        a = np.stack([noise, noise // 16, noise, ramp, ca, sa])
        b = np.stack([other, other // 16, near, ramp[..., ::-1], cb, sb])
        a.setflags(write=False), b.setflags(write=False)
        _pairs[(H, W)] = (a, b)
    return _pairs[(H, W)]


def grey_frames(H: int, W: int):
    """Two different frames of grey noise (r = g = b per pixel), uint8 H x W x 3."""
    rng = np.random.default_rng(7 * H + W)
    g1, g2 = rng.integers(0, 256, (2, H, W, 1), dtype=np.uint8)
    return np.repeat(g1, 3, axis=2), np.repeat(g2, 3, axis=2)


def checkerboard(H: int = 64, W: int = 64):
    """The README's example: a one-pixel checkerboard of codes (200, 60, 60) and (60, 200, 60), and the flat frame of its mean linear
    light, re-encoded."""
    y, x = np.mgrid[0:H, 0:W]
    board = np.where(((x + y) & 1)[..., None] == 0, np.array([200, 60, 60]), np.array([60, 200, 60])).astype(np.uint8)
    lut = decode_table()
    mean = 0.5 * (lut[[200, 60, 60]] + lut[[60, 200, 60]])
    code = [int(np.argmin(np.abs(lut - v))) for v in mean]
    return board, np.broadcast_to(np.array(code, np.uint8), (H, W, 3)).copy()
