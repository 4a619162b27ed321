"""The yardstick of the frame metrics, in float64 NumPy with explicit separable loops -- no SciPy, no code under test.

Histogram: abs_hist[c][k] = samples of channel c with |a - b| == k.  SSE and PSNR follow from it.
SSIM: Wang et al. 2004 in the form skimage computes with gaussian_weights=True, use_sample_covariance=False: per channel an 11 x 11
separable Gaussian window, sigma 1.5, taps normalised to sum 1; valid positions only (the map is (H-10) x (W-10)); C1 = (0.01*255)^2,
C2 = (0.03*255)^2; per position (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2)), s^2 = E[x^2] - mu^2;
the frame value is the mean over positions; NaN when there is no position."""
import math

import numpy as np

K, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def taps() -> np.ndarray:
    g = np.exp(-((np.arange(K, dtype=np.float64) - K // 2) ** 2) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def abs_hist(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """uint8 H x W x 3 frames -> 3 x 256 uint64."""
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return np.stack([np.bincount(d[..., c].ravel(), minlength=256) for c in range(3)]).astype(np.uint64)


def sse_from_hist(h: np.ndarray) -> list:
    return [int(sum(int(k) * int(k) * int(h[c][k]) for k in range(256))) for c in range(3)]


def psnr(sse: int, n: int) -> float:
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * n / sse)


def _window(x: np.ndarray) -> np.ndarray:
    """The valid 11 x 11 Gaussian mean of a float64 plane: rows, then columns."""
    w = taps()
    H, W = x.shape
    r = np.zeros((H, W - K + 1))
    for k in range(K):
        r += w[k] * x[:, k : k + W - K + 1]
    o = np.zeros((H - K + 1, W - K + 1))
    for k in range(K):
        o += w[k] * r[k : k + H - K + 1, :]
    return o


def ssim_plane(a: np.ndarray, b: np.ndarray) -> float:
    H, W = a.shape
    if H < K or W < K:
        return math.nan
    a, b = a.astype(np.float64), b.astype(np.float64)
    ma, mb = _window(a), _window(b)
    va, vb, cab = _window(a * a) - ma * ma, _window(b * b) - mb * mb, _window(a * b) - ma * mb
    s = ((2.0 * ma * mb + C1) * (2.0 * cab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))
    return float(s.mean())


def ssim(a: np.ndarray, b: np.ndarray) -> list:
    return [ssim_plane(a[..., c], b[..., c]) for c in range(3)]


def six_frames(H: int, W: int, seed: int = 0):
    """The six frame pairs the SSIM bound was worked out on."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pm1 = np.clip(noise.astype(np.int16) + rng.integers(-1, 2, (H, W, 3)), 0, 255).astype(np.uint8)
    ramp = np.broadcast_to(((np.arange(W) * 255) // max(1, W - 1)).astype(np.uint8)[None, :, None], (H, W, 3)).copy()
    ramp_n = np.clip(ramp.astype(np.int16) + rng.integers(-8, 9, (H, W, 3)), 0, 255).astype(np.uint8)
    flat255, flat254 = np.full((H, W, 3), 255, np.uint8), np.full((H, W, 3), 254, np.uint8)
    dot = flat255.copy()
    dot[H // 2, W // 2] = 0
    other = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return [("noise_pm1", noise, pm1), ("ramp_noise8", ramp, ramp_n), ("flat255_254", flat255, flat254), ("flat255_dot", flat255, dot),
            ("independent", noise, other), ("inverse", noise, 255 - noise)]
