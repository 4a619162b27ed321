"""The yardstick of the S-CIELAB colour difference maps in NumPy float64 -- the definition of include/avx.h, no code
under test.  Zhang & Wandell 1996: both frames are filtered in an opponent colour space by the eye's contrast sensitivity at `ppd`
pixels per degree, then CIEDE2000 is taken per pixel on the filtered frames.

1. lin = the Lab decode table of _deltae_ref applied to the three codes.   2. o = P M lin, M the sRGB -> XYZ (D65) matrix.
3. Each channel is filtered by sum_i w_i (g_i *x g_i *y o): (weight, spread in degrees) pairs per channel, a channel's weights divided
   by their sum; g[x] = exp(-x^2 / (spread ppd)^2) on x = -R .. R, R = ceil(ppd / 2), normalised to unit sum over that support; rows
   first; the border is the nearest pixel (index clamp) in both directions.
4. t = diag(1 / rowsum(M)) P^-1 o_filtered; Lab by f as in _deltae_ref, the linear branch also for negative t.  Everything here is
   float64, the inverse of P included: rounding the constants to float32 is the device's business and inside its error bound.
5. dE00 of the two Lab triples with _deltae_ref.ciede2000.
The record, the percentiles, the quantiser, the palette, the dim grey (of the unfiltered A) and the side layout (the unfiltered A and
B) are _deltae_ref's."""
import math

import numpy as np

from _deltae_ref import M, ciede2000, decode_table, pal, side  # noqa: F401

EPS, SLOPE, OFFSET = (6.0 / 29.0) ** 3, 1.0 / (3.0 * (6.0 / 29.0) ** 2), 4.0 / 29.0
P = np.array([[0.279, 0.72, -0.107], [-0.449, 0.29, -0.077], [0.086, -0.59, 0.501]])
P_INV = np.linalg.inv(P)
TERMS = (((0.921, 0.0283), (0.105, 0.133), (-0.108, 4.336)),  # luminance
         ((0.531, 0.0392), (0.330, 0.494)),                   # red-green
         ((0.488, 0.0536), (0.371, 0.386)))                   # blue-yellow
PPD_MIN, PPD_MAX = 2.0, 128.0


def radius(ppd: float) -> int:
    return int(math.ceil(ppd / 2.0))


def taps(spread: float, ppd: float) -> np.ndarray:
    """g[-R .. R] of one term, unit sum."""
    R = radius(ppd)
    x = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (spread * ppd) ** 2)
    return g / g.sum()


def weights(channel: int) -> np.ndarray:
    w = np.array([t[0] for t in TERMS[channel]], np.float64)
    return w / w.sum()


def _filter_axis(v: np.ndarray, g: np.ndarray, axis: int) -> np.ndarray:
    """The correlation of v with g along `axis`, indices clamped into the array."""
    R = len(g) // 2
    n = v.shape[axis]
    out = np.zeros_like(v)
    for k in range(-R, R + 1):
        out += g[k + R] * np.take(v, np.clip(np.arange(n) + k, 0, n - 1), axis=axis)
    return out


def opponent(rgb8: np.ndarray) -> np.ndarray:
    """uint8 (H, W, 3) -> the opponent planes (H, W, 3), float64."""
    return decode_table()[np.asarray(rgb8)] @ (P @ M).T


def filtered(rgb8: np.ndarray, ppd: float) -> np.ndarray:
    """uint8 (H, W, 3) -> the filtered opponent planes (H, W, 3)."""
    o = opponent(rgb8)
    out = np.zeros_like(o)
    for c in range(3):
        for w, (_, spread) in zip(weights(c), TERMS[c]):
            g = taps(spread, ppd)
            out[..., c] += w * _filter_axis(_filter_axis(o[..., c], g, 1), g, 0)  # rows first
    return out


def lab_of_opponent(o: np.ndarray) -> np.ndarray:
    t = (o @ P_INV.T) / M.sum(axis=1)
    f = np.where(t > EPS, np.cbrt(np.maximum(t, 0.0)), t * SLOPE + OFFSET)
    return np.stack([116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])], axis=-1)


def scielab(a8: np.ndarray, b8: np.ndarray, ppd: float) -> np.ndarray:
    """uint8 (H, W, 3) pairs -> S-CIELAB dE00, float64 (H, W)."""
    assert PPD_MIN <= ppd <= PPD_MAX and math.isfinite(ppd)
    return ciede2000(lab_of_opponent(filtered(a8, ppd)), lab_of_opponent(filtered(b8, ppd)))


# ------------------------------------------------------------------------------------------------ frames
def checkerboard(n: int = 96, lo: int = 96, hi: int = 160):
    """(a one-pixel checkerboard of codes lo / hi, the flat grey of the same mean linear light): uint8 n x n x 3 each."""
    y, x = np.mgrid[:n, :n]
    a = np.where((x + y) % 2 == 0, lo, hi).astype(np.uint8)
    lut = decode_table()
    grey = int(np.argmin(np.abs(lut - 0.5 * (lut[lo] + lut[hi]))))
    return np.repeat(a[..., None], 3, axis=2), np.full((n, n, 3), grey, np.uint8)


def frame(kind: str, H: int, W: int, seed: int) -> np.ndarray:
    """A named uint8 H x W x 3 frame: noise, dark (codes 0..23), ramp (smooth), primaries (saturated blocks of 3 x 2 pixels)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "dark":
        return rng.integers(0, 24, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[:H, :W]
    if kind == "ramp":
        return np.stack([(x * 255) // max(1, W - 1), (y * 255) // max(1, H - 1), ((x + y) * 255) // max(1, H + W - 2)], axis=-1).astype(np.uint8)
    if kind == "primaries":
        prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
        return prim[rng.integers(0, 8, ((H + 1) // 2, (W + 2) // 3))].repeat(2, axis=0).repeat(3, axis=1)[:H, :W]
    raise ValueError(kind)


def jitter(a: np.ndarray, seed: int, amp: int = 3) -> np.ndarray:
    """a with +-amp noise on every code."""
    rng = np.random.default_rng(seed)
    return np.clip(a.astype(np.int16) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)
