"""The yardstick of the difference maps in NumPy -- the definitions of include/avx.h, no code under test.

With d_c = |a_c - b_c| per channel and d = max_c d_c of a pixel, G the gain and K the threshold:
  abs:   out_c = min(255, G d_c)
  heat:  d <= K: (g, g, g), g = ((77 a_r + 150 a_g + 29 a_b + 128) >> 8) >> 2;  d > K: pal(min(255, G (d - K)))
  pal(v) = (min(255, 3v), clamp(3v - 255, 0, 255), clamp(3v - 510, 0, 255)); its sum is 3v
  ssim:  pixel (y, x) takes window position (clamp(y - 5, 0, H - 11), clamp(x - 5, 0, W - 11)) of the SSIM of _metrics_ref (11 x 11
         Gaussian window, sigma 1.5); sbar = the mean of the three channels there; v = clamp(floor(255 G (1 - sbar) + 0.5), 0, 255); pal(v)
  record: max_d, the first pixel in raster order that attains it ((0, 0) when max_d is 0), the number of pixels with d > K
ssim_positions is the float64 definition per position; map32 restates one position's float32 arithmetic operation for operation as
csrc/ssim_window.h performs it (taps rounded once, samples centred by 128, fma chains along rows and then columns, variances with the
products' rounding errors recovered), so that |map32 - ssim_positions| is the error the float32 form has by construction."""
import numpy as np

import _metrics_ref as R


def pal(v) -> np.ndarray:
    """v (integers 0..255, any shape) -> uint8 (..., 3)."""
    t = 3 * np.asarray(v).astype(np.int64)
    return np.stack([np.minimum(255, t), np.clip(t - 255, 0, 255), np.clip(t - 510, 0, 255)], axis=-1).astype(np.uint8)


def channel_diffs(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.abs(a.astype(np.int64) - b.astype(np.int64))


def abs_map(a: np.ndarray, b: np.ndarray, G: int) -> np.ndarray:
    return np.minimum(255, G * channel_diffs(a, b)).astype(np.uint8)


def heat_map(a: np.ndarray, b: np.ndarray, G: int, K: int) -> np.ndarray:
    d = channel_diffs(a, b).max(axis=-1)
    x = a.astype(np.int64)
    g = ((77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8) >> 2
    grey = np.stack([g, g, g], axis=-1).astype(np.uint8)
    hot = pal(np.minimum(255, G * np.maximum(d - K, 0)))
    return np.where((d > K)[..., None], hot, grey)


def side(a: np.ndarray, b: np.ndarray, m: np.ndarray) -> np.ndarray:
    """A | B | map along the width (the axis before the channels)."""
    return np.concatenate([a, b, m], axis=-2)


def record(a: np.ndarray, b: np.ndarray, K: int) -> tuple:
    """(max_d, max_x, max_y, beyond) of one H x W x 3 pair."""
    d = channel_diffs(a, b).max(axis=-1)
    m = int(d.max())
    y, x = (0, 0) if m == 0 else (int(v) for v in np.unravel_index(int(np.argmax(d)), d.shape))  # argmax: the first in raster order
    return m, x, y, int((d > K).sum())


# ------------------------------------------------------------------------------------------------ SSIM per position
def ssim_positions(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The float64 SSIM of every window position and channel of one H x W x 3 pair: (H - 10, W - 10, 3)."""
    out = []
    for c in range(3):
        x, y = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        ma, mb = R._window(x), R._window(y)
        va, vb, cab = R._window(x * x) - ma * ma, R._window(y * y) - mb * mb, R._window(x * y) - ma * mb
        out.append(((2.0 * ma * mb + R.C1) * (2.0 * cab + R.C2)) / ((ma * ma + mb * mb + R.C1) * (va + vb + R.C2)))
    return np.stack(out, axis=-1)


def replicate(pos: np.ndarray, H: int, W: int) -> np.ndarray:
    """Values per window position (H - 10, W - 10, ...) -> per pixel (H, W, ...): pixel (y, x) takes position (clamp(y - 5), clamp(x - 5))."""
    yy = np.clip(np.arange(H) - 5, 0, H - 11)
    xx = np.clip(np.arange(W) - 5, 0, W - 11)
    return pos[yy][:, xx]


def ssim_v_unrounded(pos64: np.ndarray, G: float) -> np.ndarray:
    """255 G (1 - sbar) per position, float64, neither rounded nor clamped."""
    return 255.0 * G * (1.0 - pos64.mean(axis=-1))


def ssim_mode_map(pos: np.ndarray, G: float, H: int, W: int) -> np.ndarray:
    """The uint8 map the definition gives for per-position values `pos` (H - 10, W - 10, 3)."""
    v = np.clip(np.floor(ssim_v_unrounded(pos.astype(np.float64), G) + 0.5), 0, 255).astype(np.int64)
    return pal(replicate(v, H, W))


_f32 = np.float32


def fma32(a, b, c) -> np.ndarray:
    """fmaf on float32 arrays, correctly rounded: the product is exact in float64; its sum with c is rounded to odd in float64 (TwoSum
    names the error), so that the final rounding to float32 is the only one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0.0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(_f32)


def _window32(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """The 11 x 11 window sums of a float32 plane as the kernels form them: w[0] * v[0], then fma(w[k], v[k], .), rows, then columns."""
    H, W = x.shape
    r = w[0] * x[:, 0 : W - 10]
    for k in range(1, 11):
        r = fma32(np.broadcast_to(w[k], r.shape), x[:, k : k + W - 10], r)
    o = w[0] * r[0 : H - 10]
    for k in range(1, 11):
        o = fma32(np.broadcast_to(w[k], o.shape), r[k : k + H - 10], o)
    return o


def map32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """One H x W x 3 pair -> float32 (H - 10, W - 10, 3): csrc/ssim_window.h's arithmetic, operation for operation."""
    w = R.taps().astype(_f32)  # each tap rounded once
    C1, C2, two, off = _f32(6.5025), _f32(58.5225), _f32(2.0), _f32(128.0)
    out = []
    for c in range(3):
        x, y = a[..., c].astype(_f32) - off, b[..., c].astype(_f32) - off
        ma, mb = _window32(x, w), _window32(y, w)
        eaa, ebb, eab = _window32(x * x, w), _window32(y * y, w), _window32(x * y, w)
        paa, pbb, pab = ma * ma, mb * mb, ma * mb
        va = (eaa - paa) - fma32(ma, ma, -paa)
        vb = (ebb - pbb) - fma32(mb, mb, -pbb)
        cab = (eab - pab) - fma32(ma, mb, -pab)
        ua, ub = ma + off, mb + off
        num = (two * (ua * ub) + C1) * (two * cab + C2)
        den = ((ua * ua + ub * ub) + C1) * ((va + vb) + C2)
        s = num / den
        assert s.dtype == _f32
        out.append(s)
    return np.stack(out, axis=-1)


def planted_pair(H: int, W: int, y0: int, x0: int, seed: int = 3):
    """b equals a, except that the 3 x 3 block at (y0, x0) is raised by 7 (a stays at most 200 there, so nothing clips)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 201, (H, W, 3), dtype=np.uint8)
    b = a.copy()
    b[y0 : y0 + 3, x0 : x0 + 3] += 7
    return a, b
