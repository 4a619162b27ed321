"""The day/night decision of DESIGN §4.23 in NumPy, for tests/test_daynight_host.py and tests/test_daynight_gpu.py.

The oracle of the decision is oracle.np_backend.NumpyProbes.median_luma(frame) < T (the restatement of RatUV._choose_mode,
animals/rat_uv.py:99-104); luma() is the Y that function forms, and record() is what avx_luma_mode_u8 must leave for a frame."""
import numpy as np

from oracle import cpu_ref as O
from oracle.np_backend import NumpyProbes

SIZES = [(1, 1), (1, 2), (2, 2), (3, 5), (13, 13), (37, 70), (96, 131), (64, 48), (270, 480)]
THRESHOLDS = [0.12, 0.0, 1.0, 0.5]
KINDS = ["black", "white", "grey30", "grey31", "half30_31", "half30_32", "half30_31_more", "half30_31_less", "half30_32_more", "half30_32_less",
         "noise", "colour", "last_below"]


def luma(frame: np.ndarray) -> np.ndarray:
    """float32 H x W: the expression of NumpyProbes.median_luma."""
    img01 = O.to_float01(frame)
    Y = 0.2126 * img01[..., 0] + 0.7152 * img01[..., 1] + 0.0722 * img01[..., 2]
    assert Y.dtype == np.float32
    return Y


def oracle_night(frame: np.ndarray, T: float) -> bool:
    return NumpyProbes.median_luma(frame) < T


def record(frame: np.ndarray, T: float):
    """(below, max_below, min_at_or_above): the count as an int, the two float32 values (0 and +inf where their set is empty)."""
    Y = luma(frame).reshape(-1)
    lo = Y.astype(np.float64) < T
    return (int(lo.sum()), np.float32(Y[lo].max()) if lo.any() else np.float32(0.0),
            np.float32(Y[~lo].min()) if (~lo).any() else np.float32(np.inf))


def _halves(H, W, a, b, moved=0):
    """The first n // 2 + moved pixels (row-major) grey a, the rest grey b."""
    n = H * W
    k = min(max(n // 2 + moved, 0), n)
    flat = np.full((n, 3), b, np.uint8)
    flat[:k] = a
    return flat.reshape(H, W, 3)


def frame(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng([seed, H, W, KINDS.index(kind)])
    if kind == "black":
        return np.zeros((H, W, 3), np.uint8)
    if kind == "white":
        return np.full((H, W, 3), 255, np.uint8)
    if kind in ("grey30", "grey31"):  # Y = 0.1176 and 0.1216: either side of 0.12
        return np.full((H, W, 3), int(kind[4:]), np.uint8)
    if kind.startswith("half30_"):  # even n: below == n / 2 at T = 0.12; the middle mean is below T with 31, above it with 32
        b = int(kind[7:9])
        moved = {"more": 1, "less": -1}.get(kind[10:], 0)  # one pixel moved: below == n / 2 + 1, n / 2 - 1
        return _halves(H, W, 30, b, moved)
    if kind == "noise":  # grey noise in codes 20..41, around the threshold
        return np.repeat(rng.integers(20, 42, (H, W, 1), dtype=np.uint8), 3, axis=2)
    if kind == "colour":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "last_below":  # the only pixel below 0.12 (and below 0.5) is the last one
        f = np.full((H, W, 3), 200, np.uint8)
        f[-1, -1] = (3, 2, 1)
        return f
    raise ValueError(kind)


def scene(mode: str, H: int, W: int, seed: int) -> np.ndarray:
    """A frame with content that is day ("D": noise in 90..255) or night ("N": noise in 0..40) at T = 0.12 by a wide margin."""
    rng = np.random.default_rng([seed, H, W, ord(mode)])
    lo, hi = (90, 256) if mode == "D" else (0, 41)
    return rng.integers(lo, hi, (H, W, 3), dtype=np.uint8)
