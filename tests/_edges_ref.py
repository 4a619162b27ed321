"""The yardstick of receptor contrast within a frame (Local Edge Intensity Analysis, van den Berg et al. 2020) in NumPy
float64 -- the definition of include/avx.h above avx_receptor_edges_u8, no code under test.

Decode: lin = _deltae_ref.decode_table()[code].  Blur (sigma != 0): _acuity_ref.blurred -- the taps, the index-order sums, rows then
columns, BORDER_REFLECT_101 -- on the one frame.  Catches: _acuity_ref.catches_of_linear, the anchored form under the row-normalised
matrix; the luminance channel is one more row, normalised the same way.  Logarithm once per pixel: f = log(q + eps).  Neighbours: the
eight offsets (+-D, 0), (0, +-D), (+-D, +-D); one outside the frame is skipped, not reflected.  df_i = f_i(p) - f_i(n); dS from the df_i
by _rnl_ref's pairs and weights; dL = |f_L(p) - f_L(n)| / e_L; v = dS, dL or the larger, by channel.  The value of a pixel is the
largest v over its neighbours inside the frame, 0 where there are none.

dtype=np.float32 restates the same operations as a float32 device forms them: the table, the taps, R', L', the weights, the reciprocal
of the denominator (K = 2: of its root) and 1 / e_L are formed in float64 and rounded once, every operation on pixels is rounded to
float32.

CASES are the sizes the tests of both files (tests/test_edges_host.py, tests/test_edges_gpu.py) run on with the (sigma, step) each is
run at, frames(H, W) the frames (the A sides of _acuity_ref.frames), ACHROMATIC the observers' luminance channels, and BOUND the accuracy the device
is held to: 8 x F32_FIGURE, the largest |float32 restatement - float64 yardstick| over all of them, which test_edges_host.py measures
and asserts."""
import numpy as np

import _acuity_ref as A
from _deltae_ref import decode_table
from _rnl_ref import PAIRS, weights

CHANNELS = ("chromatic", "achromatic", "either")
OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
KINDS = A.KINDS
# (H, W) -> the (sigma, step) it is run at.  1 x 1 has no neighbour; 1 x 9 has them along one axis only, and at step 8 one pair; 2 x 3
# and 5 x 7 are smaller than most radii and than the largest step; 16 x 16 is below one block; the owned block is 62 x 30 at D = 1,
# 60 x 28 at D = 2 and 48 x 16 at D = 8, so 33 x 70 spans blocks both ways at every step; 70 x 530 has several blocks each way, a partial
# last row and column and interior blocks whose region needs no folding; 96 x 160 has such a block at the largest radius.  Every sigma
# (0: no blur, 0.2, 1.0, 3.5, 4.0: 3, 9, 29 and 33 taps) meets every step (1, 2, 8) somewhere.
CASES = {(1, 1): ((0.0, 1), (1.0, 2), (4.0, 8)), (1, 9): ((0.0, 1), (0.2, 2), (3.5, 8)), (2, 3): ((0.0, 1), (1.0, 2), (4.0, 1)),
         (5, 7): ((0.0, 2), (0.2, 1), (3.5, 1), (4.0, 8)), (16, 16): ((0.0, 8), (1.0, 1), (4.0, 2)), (33, 70): ((0.0, 1), (0.2, 2), (3.5, 8)),
         (70, 530): ((0.0, 1), (1.0, 2), (3.5, 1), (4.0, 8)), (96, 160): ((0.0, 8), (4.0, 1))}
# the luminance channel of test_acuity_gpu.py's three observers, by name: (1-based classes, e_L).  Dog: the LM class; HoneyBee: Green;
# the four-class observer: the mean of its two long classes
ACHROMATIC = {"Dog": ((1,), 0.1), "HoneyBee": ((3,), 0.12), "four": ((1, 2), 0.08)}
# the largest |float32 restatement - float64 yardstick| over CASES x KINDS x the three observers x the three channels, rounded up from
# the 2.30e-5 that test_edges_host.py::test_float32_figure_that_sets_the_device_bound measures on a CPU (Dog, chromatic, the ramp at
# 70 x 530 without blur, step 1; the values reach 86.4, where one float32 step is 7.6e-6); the device's logf rounds differently from
# NumPy's, which is what the factor 8 is for (test_receptor_gpu.py's precedent)
F32_FIGURE = 2.5e-5
BOUND = 8 * F32_FIGURE


def frames(H: int, W: int) -> np.ndarray:
    """The six frames of a size, (6, H, W, 3) uint8, read-only: the A sides of _acuity_ref.frames."""
    return A.frames(H, W)[0]


def luminance_row(matrix, classes) -> np.ndarray:
    """The mean of the normalised rows of the 1-based `classes`, float64."""
    m = np.asarray(matrix, np.float64)
    m = m / m.sum(axis=1, keepdims=True)
    return m[[k - 1 for k in classes]].mean(axis=0)


_lin = {}


def linear(rgb8: np.ndarray, sigma: float, dtype=np.float64, key=None) -> np.ndarray:
    """uint8 (..., H, W, 3) -> the linear planes behind the blur of `sigma` pixels (0: none).  key: remember the result under it."""
    if key is not None and (key, sigma, dtype) in _lin:
        return _lin[(key, sigma, dtype)]
    lin = A.blurred(rgb8, sigma, dtype) if sigma else decode_table().astype(dtype)[np.asarray(rgb8)]
    if key is not None:
        lin.setflags(write=False)
        _lin[(key, sigma, dtype)] = lin
    return lin


def log_catches(lin: np.ndarray, rows, floor: float, dtype=np.float64) -> np.ndarray:
    """Linear (..., 3) -> f = log(q + eps) of every row of `rows` (each divided by its sum), (..., len(rows))."""
    f = np.log(A.catches_of_linear(lin, rows, dtype) + dtype(floor))
    assert f.dtype == dtype
    return f


def ds_from_contrasts(df: np.ndarray, weber, dtype=np.float64) -> np.ndarray:
    """df (..., K) -> dS (...): the forms of include/avx.h above avx_receptor_delta_u8, the pairs in that order."""
    K = df.shape[-1]
    w, den = weights(weber)
    if K == 2:
        d = np.abs(df[..., 0] - df[..., 1])
        return d / np.sqrt(den) if dtype is np.float64 else d * dtype(1.0 / np.sqrt(den))
    num = None
    for (i, j), wij in zip(PAIRS[K], w):
        d = df[..., i] - df[..., j]
        t = dtype(wij) * (d * d)
        num = t if num is None else num + t
    return np.sqrt(num / den) if dtype is np.float64 else np.sqrt(num * dtype(1.0 / den))


def pair_value(fp, fn, weber, lum_weber, channel: str, dtype=np.float64):
    """v(p, n) from the log-catches (..., K [+ 1]) of the two pixels; the luminance channel, when there is one, is the last."""
    K = len(weber)
    ds = dl = None
    if channel != "achromatic":
        ds = ds_from_contrasts(fp[..., :K] - fn[..., :K], weber, dtype)
    if channel != "chromatic":
        d = np.abs(fp[..., K] - fn[..., K])
        dl = d / lum_weber if dtype is np.float64 else d * dtype(1.0 / lum_weber)
    v = ds if dl is None else dl if ds is None else np.maximum(ds, dl)
    assert v.dtype == dtype
    return v


def values(rgb8, matrix, weber, floor, achromatic=None, channel="chromatic", sigma=0.0, step=1, dtype=np.float64, key=None) -> np.ndarray:
    """uint8 (..., H, W, 3) -> the edge value of every pixel (..., H, W).  achromatic: None or (1-based classes, e_L)."""
    assert channel in CHANNELS and (achromatic is not None or channel == "chromatic")
    rows = [list(r) for r in matrix] + ([list(luminance_row(matrix, achromatic[0]))] if achromatic is not None else [])
    f = log_catches(linear(rgb8, sigma, dtype, key), rows, floor, dtype)
    H, W = f.shape[-3], f.shape[-2]
    out = np.zeros(f.shape[:-1], dtype)
    D = step
    for dy, dx in OFFSETS:
        oy, ox = dy * D, dx * D
        ys, xs = slice(max(0, -oy), min(H, H - oy)), slice(max(0, -ox), min(W, W - ox))  # the pixels whose neighbour lies inside
        if ys.start >= ys.stop or xs.start >= xs.stop:
            continue
        yn, xn = slice(ys.start + oy, ys.stop + oy), slice(xs.start + ox, xs.stop + ox)
        v = pair_value(f[..., ys, xs, :], f[..., yn, xn, :], weber, None if achromatic is None else achromatic[1], channel, dtype)
        out[..., ys, xs] = np.maximum(out[..., ys, xs], v)
    assert out.dtype == dtype
    return out
