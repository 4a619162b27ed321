"""The yardstick of the comparison in YUV planes, in float64 NumPy with explicit separable loops -- no SciPy, no code
under test.  Planes come from _rawyuv_ref.split_planes: Y is H x W, U and V are ceil(H / 2^sy) x ceil(W / 2^sx), samples as the
decoders read them (little-endian uint16 at 10 bits, p010le shifted right by 6).

Histogram: abs_hist[p][k] = samples of plane p (Y, U, V) with |a - b| == k, 1024 bins per plane (8-bit formats use 0..255); rows of
absent planes are zero.  PSNR: 10 log10(peak^2 N / SSE) with peak = 2^d - 1, per plane and pooled over all samples of all planes.
SSIM: _metrics_ref's definition per plane at the plane's own size with dynamic range L = 2^d - 1: C1 = (0.01 L)^2, C2 = (0.03 L)^2;
NaN for an absent plane and for one smaller than 11 in either dimension.  The frame's SSIM is the planes' weighted by their sample
counts, NaN planes left out."""
import math

import numpy as np

import _metrics_ref as M
import _rawyuv_ref as Y

BINS = 1024


def planes_of(payload: np.ndarray, fmt: str, H: int, W: int):
    """One flat payload -> [Y, U, V] integer planes (None for an absent plane)."""
    y, u, v = Y.split_planes(np.asarray(payload, np.uint8).reshape(1, -1), fmt, H, W)
    return [y[0], None if u is None else u[0], None if v is None else v[0]]


def abs_hist(a: np.ndarray, b: np.ndarray, fmt_a: str, H: int, W: int, fmt_b: str = None) -> np.ndarray:
    """Two flat payloads -> 3 x 1024 uint64."""
    out = np.zeros((3, BINS), np.uint64)
    for p, (x, y) in enumerate(zip(planes_of(a, fmt_a, H, W), planes_of(b, fmt_b or fmt_a, H, W))):
        if x is not None:
            out[p] = np.bincount(np.abs(x.astype(np.int64) - y.astype(np.int64)).ravel(), minlength=BINS)
    return out


def sse_from_hist(h: np.ndarray) -> list:
    return [int(sum(int(k) * int(k) * int(h[p][k]) for k in np.nonzero(h[p])[0])) for p in range(3)]


def psnr(sse: int, n: int, depth: int) -> float:
    if n == 0:
        return math.nan
    return math.inf if sse == 0 else 10.0 * math.log10(float((1 << depth) - 1) ** 2 * n / sse)


def ssim_plane(a: np.ndarray, b: np.ndarray, L: float) -> float:
    """Mean SSIM of two integer planes of one shape with dynamic range L; NaN when there is no window position."""
    H, W = a.shape
    if H < M.K or W < M.K:
        return math.nan
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    a, b = a.astype(np.float64), b.astype(np.float64)
    ma, mb = M._window(a), M._window(b)
    va, vb, cab = M._window(a * a) - ma * ma, M._window(b * b) - mb * mb, M._window(a * b) - ma * mb
    s = ((2.0 * ma * mb + C1) * (2.0 * cab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))
    return float(s.mean())


def ssim(a: np.ndarray, b: np.ndarray, fmt_a: str, H: int, W: int, fmt_b: str = None) -> list:
    L = float((1 << Y.depth_of(fmt_a)) - 1)
    return [math.nan if x is None else ssim_plane(x, y, L)
            for x, y in zip(planes_of(a, fmt_a, H, W), planes_of(b, fmt_b or fmt_a, H, W))]


def plane_samples(fmt: str, H: int, W: int) -> tuple:
    ch, cw = Y.plane_shapes(fmt, H, W)
    return (H * W, ch * cw, ch * cw)


def ssim_mean(values, counts) -> float:
    """The planes' SSIM weighted by their sample counts; NaN planes are left out, NaN when none is left."""
    num = den = 0.0
    for v, n in zip(values, counts):
        if not math.isnan(v) and n:
            num, den = num + v * n, den + n
    return num / den if den else math.nan


def six_pairs(fmt: str, H: int, W: int, seed: int = 0):
    """The six pair kinds of _metrics_ref.six_frames at the format's depth (maximum 255 or 1023), every plane of its own size:
    noise +-1, ramp + noise, flat max against max - 1, flat max with one dot, independent, inverse -> [(name, payload a, payload b)],
    flat uint8 payloads of `fmt`."""
    d = Y.depth_of(fmt)
    top = (1 << d) - 1
    rng = np.random.default_rng(seed)
    ch, cw = Y.plane_shapes(fmt, H, W)
    shapes = [(H, W)] + ([(ch, cw), (ch, cw)] if ch else [])

    def build(kind):
        A, B = [], []
        for h, w in shapes:
            noise = rng.integers(0, top + 1, (h, w))
            if kind == "noise_pm1":
                a, b = noise, np.clip(noise + rng.integers(-1, 2, (h, w)), 0, top)
            elif kind == "ramp_noise8":
                a = np.broadcast_to(((np.arange(w) * top) // max(1, w - 1))[None, :], (h, w)).copy()
                b = np.clip(a + rng.integers(-8, 9, (h, w)) * (1 << (d - 8)), 0, top)
            elif kind == "flatmax_maxm1":
                a, b = np.full((h, w), top), np.full((h, w), top - 1)
            elif kind == "flatmax_dot":
                a = np.full((h, w), top)
                b = a.copy()
                b[h // 2, w // 2] = 0
            elif kind == "independent":
                a, b = noise, rng.integers(0, top + 1, (h, w))
            else:
                a, b = noise, top - noise
            A.append(a[None].astype(np.int64))
            B.append(b[None].astype(np.int64))
        if not ch:
            A, B = A + [None, None], B + [None, None]
        return Y.join_planes(A[0], A[1], A[2], fmt)[0], Y.join_planes(B[0], B[1], B[2], fmt)[0]

    return [(k,) + build(k) for k in ("noise_pm1", "ramp_noise8", "flatmax_maxm1", "flatmax_dot", "independent", "inverse")]
