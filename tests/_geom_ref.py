"""Float64 NumPy statements of the geometric operations of csrc/geom.hip, written from their mathematical definitions alone
(no table construction, no fixed point, no float32 intermediate): what oracle/cvref.cpp is measured against.

resize: separable; each axis is a (destination x source) weight matrix, the two applied one after the other.
sobel: 3x3 derivative / smoothing kernels over reflect-101 padding.  remap: bilinear over a constant border at coordinates
quantised to 1/32 px.  split: left half of one frame, right half of the other, optional white seam column."""
import numpy as np

INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA = 0, 1, 2, 3


def _centres(s: int, d: int) -> np.ndarray:
    """Source coordinate of each destination pixel centre: (i + 0.5) s / d - 0.5."""
    return (np.arange(d, dtype=np.float64) + 0.5) * s / d - 0.5


def _scatter(d: int, s: int, taps: np.ndarray, w: np.ndarray) -> np.ndarray:
    """Weight matrix from per-destination taps (d, k) and weights (d, k); taps outside [0, s) replicate the border."""
    M = np.zeros((d, s), np.float64)
    np.add.at(M, (np.arange(d)[:, None], np.clip(taps, 0, s - 1)), w)
    return M


def nearest_matrix(s: int, d: int) -> np.ndarray:
    """min(floor(i * (s / d)), s - 1).  The scale s / d is one float64 number, as in cv2: where i s / d is an integer in exact
    arithmetic the float64 product can fall just below it (84 -> 1920: 160 * (84 / 1920) = 6.999..., exactly 7), and cv2 floors that."""
    src = np.minimum(np.floor(np.arange(d, dtype=np.float64) * (s / d)).astype(np.int64), s - 1)
    return _scatter(d, s, src[:, None], np.ones((d, 1)))


def linear_matrix(s: int, d: int) -> np.ndarray:
    x = _centres(s, d)
    i = np.floor(x).astype(np.int64)
    t = x - i
    return _scatter(d, s, np.stack([i, i + 1], 1), np.stack([1 - t, t], 1))


def keys(t: np.ndarray, a: float = -0.75) -> np.ndarray:
    """The Keys cubic convolution kernel."""
    t = np.abs(t)
    return np.where(t <= 1, ((a + 2) * t - (a + 3)) * t * t + 1, np.where(t < 2, ((a * t - 5 * a) * t + 8 * a) * t - 4 * a, 0.0))


def cubic_matrix(s: int, d: int) -> np.ndarray:
    x = _centres(s, d)
    i = np.floor(x).astype(np.int64)
    taps = i[:, None] + np.arange(-1, 3)[None, :]
    return _scatter(d, s, taps, keys(x[:, None] - taps))


def area_matrix(s: int, d: int) -> np.ndarray:
    """Box overlap of destination cell [i s/d, (i+1) s/d) (clipped to the source) with each unit source cell, over the clipped cell."""
    lo = np.arange(d, dtype=np.float64) * s / d
    hi = np.minimum(lo + s / d, float(s))
    k = np.arange(s, dtype=np.float64)[None, :]
    ov = np.clip(np.minimum(hi[:, None], k + 1) - np.maximum(lo[:, None], k), 0.0, None)
    return ov / (hi - lo)[:, None]


def resize64(img: np.ndarray, dsize, interp: int) -> np.ndarray:
    """cv2.resize(img, (Wd, Hd), interpolation=interp) in float64 for an HxW or HxWxC image of any dtype."""
    Wd, Hd = int(dsize[0]), int(dsize[1])
    a = np.asarray(img, np.float64)
    H, W = a.shape[:2]
    if interp == INTER_AREA and (Wd > W or Hd > H):
        interp = INTER_LINEAR
    mat = {INTER_NEAREST: nearest_matrix, INTER_LINEAR: linear_matrix, INTER_CUBIC: cubic_matrix, INTER_AREA: area_matrix}[interp]
    rows = np.tensordot(mat(W, Wd), a, axes=([1], [1]))  # (Wd, H, ...): the horizontal pass
    rows = np.moveaxis(rows, 0, 1)                        # (H, Wd, ...)
    return np.tensordot(mat(H, Hd), rows, axes=([1], [0]))  # (Hd, Wd, ...): the vertical pass


def _reflect101(i: np.ndarray, n: int) -> np.ndarray:
    """Index of reflect-101 padding (dcb|abcd|cba); a length-1 axis reflects to itself."""
    if n == 1:
        return np.zeros_like(i)
    i = np.abs(i) % (2 * (n - 1))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def sobel64(p: np.ndarray):
    """(gx, gy) of the 3x3 Sobel operator with reflect-101 padding: derivative [-1 0 1] along one axis, smoothing [1 2 1] along the other."""
    a = np.asarray(p, np.float64)
    H, W = a.shape
    q = a[_reflect101(np.arange(-1, H + 1), H)][:, _reflect101(np.arange(-1, W + 1), W)]
    dx = q[:, 2:] - q[:, :-2]
    sx = q[:, :-2] + 2 * q[:, 1:-1] + q[:, 2:]
    return dx[:-2] + 2 * dx[1:-1] + dx[2:], sx[2:] - sx[:-2]


def remap64(img: np.ndarray, mx: np.ndarray, my: np.ndarray, border: float = 0.0) -> np.ndarray:
    """cv2.remap(img, mx, my, INTER_LINEAR, BORDER_CONSTANT, border) in float64 for HxW or HxWxC.  Each coordinate is quantised to
    q = rint(32 v); a NaN or a q outside [-2^31, 2^31) on either axis gives the border value."""
    a = np.asarray(img, np.float64)
    flat = a.ndim == 2
    a = a[..., None] if flat else a
    H, W, C = a.shape
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = np.rint(np.asarray(mx, np.float64) * 32.0), np.rint(np.asarray(my, np.float64) * 32.0)
        ok = (qx >= -2.0 ** 31) & (qx < 2.0 ** 31) & (qy >= -2.0 ** 31) & (qy < 2.0 ** 31)  # False for NaN
    qx, qy = np.where(ok, qx, 0.0), np.where(ok, qy, 0.0)
    ix, iy = np.floor(qx / 32.0).astype(np.int64), np.floor(qy / 32.0).astype(np.int64)
    tx, ty = (qx / 32.0 - ix)[..., None], (qy / 32.0 - iy)[..., None]
    pad = np.full((H + 2, W + 2, C), float(border), np.float64)  # one border pixel all round; anything further out is border too
    pad[1:-1, 1:-1] = a

    def at(yy, xx):
        return pad[np.clip(yy + 1, 0, H + 1), np.clip(xx + 1, 0, W + 1)]

    out = (at(iy, ix) * (1 - tx) + at(iy, ix + 1) * tx) * (1 - ty) + (at(iy + 1, ix) * (1 - tx) + at(iy + 1, ix + 1) * tx) * ty
    out = np.where(ok[..., None], out, float(border))
    return out[..., 0] if flat else out


def split64(orig: np.ndarray, mod: np.ndarray, seam: bool) -> np.ndarray:
    """Left W // 2 columns of `orig`, the rest of `mod`; column W // 2 white when `seam`."""
    W = orig.shape[1]
    out = np.concatenate([orig[:, : W // 2], mod[:, W // 2:]], axis=1)
    if seam:
        out[:, W // 2] = 255
    return out
