"""The yardstick of the colour difference maps in NumPy float64 -- the definition of include/avx.h, no code under test.

Lab of an 8-bit sRGB pixel: lin(code) = c / 12.92 where c = code / 255 <= 0.04045, else ((c + 0.055) / 1.055) ** 2.4; M' = the sRGB -> XYZ
(D65) matrix with every row divided by its own sum; t_i = g + M'_i0 (r - g) + M'_i2 (b - g) (the form anchored on green: greys have
t_X = t_Y = t_Z exactly); f(t) = cbrt(t) where t > (6/29)^3, else t / (3 (6/29)^2) + 4/29; L = 116 f_Y - 16, a = 500 (f_X - f_Y),
b = 200 (f_Y - f_Z).  dE00: Sharma, Wu, Dalal 2005, k_L = k_C = k_H = 1.  Equal codes give exactly 0.
The record: hist[k] = pixels with min(255, floor(2 dE)) == k, the sum, the largest dE with the first pixel in raster order that attains
it, the pixels with dE > T.  percentile(q) = the upper edge (k + 1) / 2 of the first bin whose cumulative count reaches ceil(q H W), and
max_de where that is the open last bin.  The map quantiser is float32 with one rounding per operation (no fused multiply-add):
heat: dE <= T: the dim grey of A, else pal(min(255, floor(G (dE - T) + 0.5))); plain: pal(min(255, floor(G dE + 0.5)))."""
import math

import numpy as np

from _diff_ref import pal, side  # noqa: F401  (the palette and the A | B | map layout are diff's)

M = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]])
MP = M / M.sum(axis=1, keepdims=True)
EPS, SLOPE, OFFSET = (6.0 / 29.0) ** 3, 1.0 / (3.0 * (6.0 / 29.0) ** 2), 4.0 / 29.0


def decode_table() -> np.ndarray:
    """lin(code) for the 256 codes, float64."""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def lab(rgb8: np.ndarray, dtype=np.float64) -> np.ndarray:
    """uint8 (..., 3) -> Lab (..., 3).  dtype float32 restates the anchored form as a float32 device forms it: the table rounded once,
    every operation rounded to float32."""
    lut = decode_table().astype(dtype)
    mp = MP.astype(dtype)
    lin = lut[np.asarray(rgb8)]
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    dr, db = r - g, b - g
    t = [(g + mp[i, 0] * dr) + mp[i, 2] * db for i in range(3)]
    f = [np.where(v > dtype(EPS), np.cbrt(v), v * dtype(SLOPE) + dtype(OFFSET)) for v in t]
    out = np.stack([dtype(116.0) * f[1] - dtype(16.0), dtype(500.0) * (f[0] - f[1]), dtype(200.0) * (f[1] - f[2])], axis=-1)
    assert out.dtype == dtype
    return out


def hues(lab1: np.ndarray, lab2: np.ndarray):
    """(h'1, h'2, C'1 C'2) in degrees, as ciede2000 forms them."""
    a1, b1, a2, b2 = lab1[..., 1], lab1[..., 2], lab2[..., 1], lab2[..., 2]
    cb7 = (0.5 * (np.hypot(a1, b1) + np.hypot(a2, b2))) ** 7
    g = 0.5 * (1.0 - np.sqrt(cb7 / (cb7 + 25.0 ** 7)))
    a1p, a2p = (1.0 + g) * a1, (1.0 + g) * a2
    h1 = np.where((a1p == 0) & (b1 == 0), 0.0, np.degrees(np.arctan2(b1, a1p)) % 360.0)
    h2 = np.where((a2p == 0) & (b2 == 0), 0.0, np.degrees(np.arctan2(b2, a2p)) % 360.0)
    return h1, h2, np.hypot(a1p, b1), np.hypot(a2p, b2)


def ciede2000(lab1: np.ndarray, lab2: np.ndarray) -> np.ndarray:
    """Sharma, Wu, Dalal 2005 with k_L = k_C = k_H = 1, float64, on (..., 3) Lab arrays."""
    lab1, lab2 = np.asarray(lab1, np.float64), np.asarray(lab2, np.float64)
    L1, L2 = lab1[..., 0], lab2[..., 0]
    h1, h2, c1p, c2p = hues(lab1, lab2)
    cc = c1p * c2p
    dL, dC = L2 - L1, c2p - c1p
    d = h2 - h1
    dh = np.where(cc == 0, 0.0, np.where(d > 180.0, d - 360.0, np.where(d < -180.0, d + 360.0, d)))
    dH = 2.0 * np.sqrt(cc) * np.sin(np.radians(dh) / 2.0)
    Lb, Cb = 0.5 * (L1 + L2), 0.5 * (c1p + c2p)
    s = h1 + h2
    hb = np.where(cc == 0, s, np.where(np.abs(h1 - h2) <= 180.0, 0.5 * s, np.where(s < 360.0, 0.5 * (s + 360.0), 0.5 * (s - 360.0))))
    T = (1.0 - 0.17 * np.cos(np.radians(hb - 30.0)) + 0.24 * np.cos(np.radians(2.0 * hb)) + 0.32 * np.cos(np.radians(3.0 * hb + 6.0))
         - 0.20 * np.cos(np.radians(4.0 * hb - 63.0)))
    dtheta = 30.0 * np.exp(-(((hb - 275.0) / 25.0) ** 2))
    cb7 = Cb ** 7
    RC = 2.0 * np.sqrt(cb7 / (cb7 + 25.0 ** 7))
    lm2 = (Lb - 50.0) ** 2
    SL = 1.0 + 0.015 * lm2 / np.sqrt(20.0 + lm2)
    SC, SH = 1.0 + 0.045 * Cb, 1.0 + 0.015 * Cb * T
    RT = -np.sin(np.radians(2.0 * dtheta)) * RC
    tL, tC, tH = dL / SL, dC / SC, dH / SH
    return np.sqrt(np.maximum(0.0, tL * tL + tC * tC + tH * tH + RT * tC * tH))


def delta_e(a8: np.ndarray, b8: np.ndarray) -> np.ndarray:
    """uint8 (..., 3) pairs -> dE00 float64 (...); exactly 0 where the codes are equal."""
    a8, b8 = np.asarray(a8), np.asarray(b8)
    de = ciede2000(lab(a8), lab(b8))
    return np.where((a8 == b8).all(axis=-1), 0.0, de)


def hue_ambiguous(a8: np.ndarray, b8: np.ndarray, tol_deg: float = 1e-3) -> np.ndarray:
    """Where | |h'1 - h'2| - 180 | < tol_deg with both chromas non-zero: the mean-hue rule is discontinuous there and either side is a
    correct evaluation."""
    h1, h2, c1p, c2p = hues(lab(np.asarray(a8)), lab(np.asarray(b8)))
    return (np.abs(np.abs(h1 - h2) - 180.0) < tol_deg) & (c1p * c2p != 0)


# ------------------------------------------------------------------------------------------------ the record
def record(v: np.ndarray, T: float) -> dict:
    """The record of one frame's float32 values v (H x W): hist, sum (float64), max_de, max_x, max_y, beyond."""
    v = np.asarray(v)
    assert v.dtype == np.float32 and v.ndim == 2
    bins = np.minimum(255, np.floor(2.0 * v.astype(np.float64)).astype(np.int64))
    m = v.max()
    y, x = (0, 0) if m == 0 else (int(i) for i in np.unravel_index(int(np.argmax(v)), v.shape))  # argmax: the first in raster order
    return dict(hist=np.bincount(bins.ravel(), minlength=256).astype(np.uint64), sum=float(v.astype(np.float64).sum()), max_de=float(m), max_x=x,
                max_y=y, beyond=int((v > np.float32(T)).sum()))


def percentile(hist, max_de: float, q: float) -> float:
    """The upper edge (k + 1) / 2 of the first bin k whose cumulative count reaches ceil(q N); max_de where that is the last bin."""
    hist = [int(h) for h in hist]
    need, run = math.ceil(q * sum(hist)), 0
    for k, h in enumerate(hist):
        run += h
        if run >= need:
            return float(max_de) if k == 255 else (k + 1) / 2.0
    return float(max_de)


# ------------------------------------------------------------------------------------------------ the map
def quantise(v: np.ndarray, G: float, T: float, mode: str) -> np.ndarray:
    """float32 values -> the palette index 0..255 (int64), one float32 rounding per operation."""
    v, G, T = np.asarray(v, np.float32), np.float32(G), np.float32(T)
    x = v - T if mode == "heat" else v
    q = np.floor(G * x + np.float32(0.5))
    assert q.dtype == np.float32
    return np.clip(q, 0, 255).astype(np.int64)


def de_map(v: np.ndarray, a8: np.ndarray, G: float, T: float, mode: str) -> np.ndarray:
    """The uint8 map (..., 3) of float32 values v (...) over frame a8 (..., 3)."""
    hot = pal(quantise(v, G, T, mode))
    if mode == "plain":
        return hot
    x = np.asarray(a8).astype(np.int64)
    g = ((77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8) >> 2
    grey = np.stack([g, g, g], axis=-1).astype(np.uint8)
    return np.where((np.asarray(v, np.float32) > np.float32(T))[..., None], hot, grey)


# ------------------------------------------------------------------------------------------------ frames
CORNERS = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
SATURATED = np.array([[0, 0, 255], [255, 0, 0], [0, 255, 0], [0, 0, 128], [255, 0, 255], [0, 255, 255], [255, 255, 0], [40, 0, 255]], np.uint8)


def frames(H: int, W: int, seed: int):
    """The named frame pairs of a size: [(name, a, b)], uint8 H x W x 3, read-only."""
    rng = np.random.default_rng(seed)
    n = H * W
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    near = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    other = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    i = np.arange(n)
    grey = np.repeat((i % 256).astype(np.uint8)[:, None], 3, axis=1).reshape(H, W, 3)  # all 256 greys once n >= 256
    sat = SATURATED[(i // 256) % len(SATURATED)].reshape(H, W, 3)
    ca, cb = CORNERS[(i // 8) % 8].reshape(H, W, 3), CORNERS[i % 8].reshape(H, W, 3)  # all 8 x 8 pairs once n >= 64
    out = [("near", a, near), ("random", a, other), ("grey-saturated", grey, sat), ("saturated-grey", sat, grey), ("corners", ca, cb), ("same", a, a.copy())]
    for _, x, y in out:
        x.setflags(write=False), y.setflags(write=False)
    return out
