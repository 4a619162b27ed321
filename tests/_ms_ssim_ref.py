"""The yardstick of MS-SSIM (Wang, Simoncelli, Bovik 2003), in float64 NumPy on the window and constants of
tests/_metrics_ref.py -- no SciPy, no code under test.

Per channel of two uint8 H x W x 3 frames.  Five scales: scale 0 is the channel as float64, scale j + 1 the 2 x 2 mean of scale j at
floor(h / 2) x floor(w / 2), a trailing odd row or column dropped (equivalently: the sum of an origin-aligned 2^j x 2^j block divided by
4^j, block_sums below).  At every scale the 11 x 11 Gaussian window (sigma 1.5, valid positions, L = 255) gives per position
cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2) and l = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1); cs[j] is the mean of cs, ssim[j] the
mean of l * cs.  MS-SSIM = prod_{j<4} max(cs[j], 0)^w_j * max(ssim[4], 0)^w_4, the clamp being TensorFlow's and pytorch-msssim's
convention (the stored means are not clamped); the frame value is the mean of the three channels.  Scale 4 needs one window position:
H >= 176 and W >= 176, smaller frames are a ValueError."""
import numpy as np

from _metrics_ref import C1, C2, K, _window

SCALES = 5
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIDE = K << (SCALES - 1)  # 176


def pool2(x: np.ndarray) -> np.ndarray:
    """The 2 x 2 mean at floor(h / 2) x floor(w / 2)."""
    h, w = x.shape[0] // 2, x.shape[1] // 2
    x = x[: 2 * h, : 2 * w]
    return (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2]) / 4.0


def pyramid(x: np.ndarray) -> list:
    """The five scales of one uint8 plane, float64, by successive pooling."""
    if x.ndim != 2 or x.shape[0] < MIN_SIDE or x.shape[1] < MIN_SIDE:
        raise ValueError(f"five scales need a plane of at least {MIN_SIDE} x {MIN_SIDE} (got {x.shape})")
    out = [x.astype(np.float64)]
    for _ in range(SCALES - 1):
        out.append(pool2(out[-1]))
    return out


def block_sums(x: np.ndarray, j: int) -> np.ndarray:
    """Scale j of a uint8 plane as integer sums of origin-aligned 2^j x 2^j blocks (to be divided by 4^j); at most 255 * 4^j."""
    n = 1 << j
    h, w = x.shape[0] >> j, x.shape[1] >> j
    return x[: h * n, : w * n].astype(np.int64).reshape(h, n, w, n).sum(axis=(1, 3))


def scale_terms(a: np.ndarray, b: np.ndarray):
    """(mean cs, mean l * cs) of two float64 planes of one scale."""
    ma, mb = _window(a), _window(b)
    va, vb, cab = _window(a * a) - ma * ma, _window(b * b) - mb * mb, _window(a * b) - ma * mb
    cs = (2.0 * cab + C2) / (va + vb + C2)
    l = (2.0 * ma * mb + C1) / (ma * ma + mb * mb + C1)
    return float(cs.mean()), float((l * cs).mean())


def levels(a: np.ndarray, b: np.ndarray):
    """uint8 H x W x 3 frames -> (cs, ssim), each 3 x 5 float64: [channel][scale]."""
    cs, ss = np.zeros((3, SCALES)), np.zeros((3, SCALES))
    for c in range(3):
        for j, (pa, pb) in enumerate(zip(pyramid(a[..., c]), pyramid(b[..., c]))):
            cs[c, j], ss[c, j] = scale_terms(pa, pb)
    return cs, ss


def combine(cs, ssim) -> float:
    """The product formula on one channel's five cs means and five ssim means."""
    v = max(float(ssim[SCALES - 1]), 0.0) ** WEIGHTS[SCALES - 1]
    for j in range(SCALES - 1):
        v *= max(float(cs[j]), 0.0) ** WEIGHTS[j]
    return v


def ms_ssim_channels(a: np.ndarray, b: np.ndarray) -> list:
    cs, ss = levels(a, b)
    return [combine(cs[c], ss[c]) for c in range(3)]


def ms_ssim(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.mean(ms_ssim_channels(a, b)))
