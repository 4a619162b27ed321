"""The yardstick of the edge-preserving smoothing in receptor space in front of the edges in NumPy float64 -- the
definition of include/avx.h above avx_receptor_edges_smooth_u8, no code under test; everything up to the planes of log-catches and
the pair value v(p, n) is _edges_ref's.

One iteration, for every pixel p of every plane at once, from the planes of the iteration before: the window is the pixels n inside the
frame with |dx| <= R and |dy| <= R (p included, N of them; outside the frame: skipped); m = ceil(KEEP N) in float64; t = the m-th
smallest v(p, n) of the window; h = t + t; h = 0: w_n = 1 where v(p, n) = 0 else 0; otherwise rh = 1 / h, u = v(p, n) rh, a = 1 - u u,
w_n = a a where u < 1 else 0; f'(p) = f(p) + sum(w_n (f(n) - f(p))) / sum(w_n), both sums from 0 in raster order of the window (dy
outer, dx inner).  ITER iterations, then _edges_ref's neighbour contrasts on the result.  The planes are carried as the K receptor
planes and, where the observer has a luminance channel, that plane behind them, whatever the channel: the weights come from the
channel's v alone, so the planes of the channel are the device's and the others are ignored (channel_planes picks the channel's).

dtype=np.float32 restates the same operations as a float32 device forms them, in the style of _edges_ref: every operation on pixels
is rounded to float32; the selection is exact in both.

SETTINGS are the (R, KEEP, ITER) the tests run, CASES the sizes with the (setting, sigma, step) each is run at: every setting meets
every size class -- 1 x 1 (N = 1), 1 x 9, {2 x 3, 5 x 7} (the window of R = 5 is larger than the frame), 16 x 16 (below one tile),
{33 x 70, 70 x 130} (several tiles each way, partial last ones) -- somewhere, at sigma 0 and 1.0 and steps 1 and 8.  BOUND is the
accuracy the device is held to: 8 x F32_FIGURE, the largest |float32 restatement - float64 yardstick| over all of them -- of the edge
values, and of the smoothed planes in the observer's own metric, v(f'_32(p), f'_64(p)) -- which test_edges_smooth_host.py measures
and asserts.  No pixel is exempted anywhere: the weights taper to zero at the bandwidth, so the definition is continuous."""
import math

import numpy as np

import _edges_ref as E

SETTINGS = ((1, 0.5, 2), (3, 0.3, 1), (5, 0.33, 3), (2, 1.0, 1), (5, 0.01, 1))  # the last: m = 1, t = 0
_S = SETTINGS
CASES = {(1, 1): ((_S[0], 0.0, 1), (_S[1], 1.0, 8), (_S[2], 0.0, 1), (_S[3], 1.0, 1), (_S[4], 0.0, 8)),
         (1, 9): ((_S[0], 1.0, 1), (_S[1], 0.0, 8), (_S[2], 1.0, 1), (_S[3], 0.0, 1), (_S[4], 1.0, 8)),
         (2, 3): ((_S[0], 0.0, 1), (_S[2], 1.0, 1), (_S[4], 0.0, 1)),
         (5, 7): ((_S[0], 1.0, 1), (_S[1], 1.0, 1), (_S[2], 0.0, 8), (_S[3], 0.0, 1)),
         (16, 16): ((_S[0], 0.0, 8), (_S[1], 1.0, 1), (_S[2], 0.0, 1), (_S[3], 1.0, 8), (_S[4], 0.0, 1)),
         (33, 70): ((_S[0], 1.0, 8), (_S[2], 0.0, 1), (_S[3], 0.0, 1), (_S[4], 1.0, 1)),
         (70, 130): ((_S[0], 0.0, 1), (_S[1], 1.0, 8), (_S[3], 0.0, 1), (_S[4], 1.0, 1))}
MAX_WINDOW = 121
# the largest |float32 restatement - float64 yardstick| over CASES x KINDS x the three observers x the three channels, rounded up from
# what test_edges_smooth_host.py::test_float32_figure_that_sets_the_device_bound measures on a CPU: 1.343e-4 for the edge values and
# 1.268e-4 for the planes in the observer's metric (both: the four-class observer, chromatic, 33 x 70 at (5, 0.33, 3) without blur,
# step 1); the values reach 86.4, where one float32 step is 7.6e-6, and three iterations of 121-term sums carry the roundings on
F32_FIGURE = 1.5e-4
BOUND = 8 * F32_FIGURE


def rank_table(keep: float):
    """m = ceil(KEEP N) for N = 0 .. 121, in float64 as the host forms it."""
    return np.array([math.ceil(keep * float(n)) for n in range(MAX_WINDOW + 1)], np.int64)


def log_planes(rgb8, matrix, weber, floor, achromatic=None, sigma=0.0, dtype=np.float64, key=None) -> np.ndarray:
    """uint8 (..., H, W, 3) -> f (..., H, W, K [+ 1]): the log-catches of _edges_ref.values, the luminance plane last."""
    rows = [list(r) for r in matrix] + ([list(E.luminance_row(matrix, achromatic[0]))] if achromatic is not None else [])
    return E.log_catches(E.linear(rgb8, sigma, dtype, key), rows, floor, dtype)


def _window(H, W, R):
    """The window's offsets in raster order with the slices of the pixels whose neighbour lies inside and of those neighbours."""
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
            if ys.start < ys.stop and xs.start < xs.stop:
                yield ys, xs, slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)


def smooth_once(f, weber, lum_weber, channel, R, keep, dtype=np.float64) -> np.ndarray:
    H, W = f.shape[-3], f.shape[-2]
    win = list(_window(H, W, R))
    v = np.full((len(win),) + f.shape[:-1], np.inf, dtype)
    for k, (ys, xs, yn, xn) in enumerate(win):
        v[k][..., ys, xs] = E.pair_value(f[..., ys, xs, :], f[..., yn, xn, :], weber, lum_weber, channel, dtype)
    n = np.isfinite(v).sum(axis=0)
    m = rank_table(keep)[n]
    assert (m >= 1).all() and (m <= n).all()
    t = np.take_along_axis(np.sort(v, axis=0), (m - 1)[None], axis=0)[0]
    h = t + t
    with np.errstate(divide="ignore", invalid="ignore"):
        rh = dtype(1.0) / h
    sw = np.zeros(f.shape[:-1], dtype)
    acc = np.zeros(f.shape, dtype)
    for k, (ys, xs, yn, xn) in enumerate(win):
        vk, hk = v[k][..., ys, xs], h[..., ys, xs]
        with np.errstate(invalid="ignore", over="ignore"):
            u = vk * rh[..., ys, xs]
            a = dtype(1.0) - u * u
            w = np.where(hk == 0, np.where(vk == 0, dtype(1.0), dtype(0.0)), np.where(u < 1, a * a, dtype(0.0))).astype(dtype)
        sw[..., ys, xs] = sw[..., ys, xs] + w
        acc[..., ys, xs, :] = acc[..., ys, xs, :] + w[..., None] * (f[..., yn, xn, :] - f[..., ys, xs, :])
    out = f + acc / sw[..., None]
    assert out.dtype == dtype and (sw >= 1).all()
    return out


def smoothed(f, weber, lum_weber, channel, smooth, dtype=np.float64) -> np.ndarray:
    R, keep, iterations = smooth
    for _ in range(iterations):
        f = smooth_once(f, weber, lum_weber, channel, R, keep, dtype)
    return f


def channel_planes(f, K: int, channel: str) -> np.ndarray:
    """f (..., H, W, K [+ 1]) -> the channel's planes as the library returns them, (..., P, H, W)."""
    sel = f[..., :K] if channel == "chromatic" else f[..., K:] if channel == "achromatic" else f
    return np.ascontiguousarray(np.moveaxis(sel, -1, -3))


def edge_values(f, weber, lum_weber, channel, step, dtype=np.float64) -> np.ndarray:
    """_edges_ref.values' neighbour walk, from the planes."""
    H, W = f.shape[-3], f.shape[-2]
    out = np.zeros(f.shape[:-1], dtype)
    for dy, dx in E.OFFSETS:
        oy, ox = dy * step, dx * step
        ys, xs = slice(max(0, -oy), min(H, H - oy)), slice(max(0, -ox), min(W, W - ox))
        if ys.start >= ys.stop or xs.start >= xs.stop:
            continue
        yn, xn = slice(ys.start + oy, ys.stop + oy), slice(xs.start + ox, xs.stop + ox)
        out[..., ys, xs] = np.maximum(out[..., ys, xs], E.pair_value(f[..., ys, xs, :], f[..., yn, xn, :], weber, lum_weber, channel, dtype))
    assert out.dtype == dtype
    return out


def planes_and_values(rgb8, matrix, weber, floor, achromatic, channel, sigma, step, smooth, dtype=np.float64, key=None):
    """uint8 (..., H, W, 3) -> (the smoothed planes of the channel (..., P, H, W), the edge values (..., H, W), all the planes
    (..., H, W, K [+ 1]) for the observer's metric)."""
    assert channel in E.CHANNELS and (achromatic is not None or channel == "chromatic")
    lum_weber = None if achromatic is None else achromatic[1]
    f = smoothed(log_planes(rgb8, matrix, weber, floor, achromatic, sigma, dtype, key), weber, lum_weber, channel, smooth, dtype)
    return channel_planes(f, len(weber), channel), edge_values(f, weber, lum_weber, channel, step, dtype), f


def plane_error(got, want, K, weber, lum_weber, channel) -> np.ndarray:
    """The error of planes (..., P, H, W) against float64 planes of the same shape, in the observer's metric: v(got(p), want(p)) per
    pixel, float64."""
    g, w = np.moveaxis(got.astype(np.float64), -3, -1), np.moveaxis(want, -3, -1)
    if channel == "achromatic":  # pair_value reads the luminance plane behind K receptor planes
        pad = np.zeros(g.shape[:-1] + (K,))
        g, w = np.concatenate([pad, g], axis=-1), np.concatenate([pad, w], axis=-1)
    return E.pair_value(g, w, weber, lum_weber, channel)
