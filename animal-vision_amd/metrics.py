"""Frame comparison on the device (csrc/metrics.hip): what two uint8 RGB frames differ by -- per channel the exact
histogram of absolute code differences (from which SSE, PSNR, the largest difference and the share of samples beyond +-k codes follow
on the host without rounding) and the mean SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid positions only; the form
skimage computes with gaussian_weights=True, use_sample_covariance=False).

frame_metrics_device works on frames that are on the device already; frame_metrics takes arrays.  python -m animal_vision_amd.compare
is the command built on them."""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional

import numpy as np

from ._lib import AVX_METRICS_MAX_FRAMES, FrameMetricsRecord, lib
from .runtime import Context, DeviceBuffer, get_context

MAX_FRAMES = AVX_METRICS_MAX_FRAMES
RECORD_BYTES = ctypes.sizeof(FrameMetricsRecord)  # 3 * 256 uint32, then 3 doubles
_RECORD_DTYPE = np.dtype([("abs_hist", np.uint32, (3, 256)), ("ssim", np.float64, (3,))])
assert _RECORD_DTYPE.itemsize == RECORD_BYTES
_K2 = np.arange(256, dtype=np.uint64) ** 2


def _psnr(sse: int, n: int) -> float:
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * n / sse)


class FrameMetrics:
    """One frame's record: abs_hist[c][k] = samples of channel c with |a - b| == k (3 x 256 uint64), ssim[c] = mean SSIM of channel c
    (NaN where it was not computed).  Everything else is derived from the histogram here, in integers where it is a count."""

    __slots__ = ("abs_hist", "ssim")

    def __init__(self, abs_hist, ssim=(math.nan, math.nan, math.nan)):
        h = np.asarray(abs_hist)
        if h.shape != (3, 256):
            raise ValueError(f"abs_hist is 3 x 256 (got {h.shape})")
        self.abs_hist = h.astype(np.uint64)
        self.ssim = tuple(float(v) for v in ssim)
        if len(self.ssim) != 3:
            raise ValueError(f"ssim holds three values (got {len(self.ssim)})")

    @property
    def samples(self) -> int:
        """Samples per channel (H * W)."""
        return int(self.abs_hist[0].sum())

    @property
    def sse(self) -> tuple:
        """Per channel: the sum of squared differences, sum_k k^2 * hist[c][k]."""
        return tuple(int((self.abs_hist[c] * _K2).sum()) for c in range(3))

    @property
    def psnr_channels(self) -> tuple:
        """Per channel: 10 log10(255^2 N / SSE), inf at SSE = 0."""
        return tuple(_psnr(s, self.samples) for s in self.sse)

    @property
    def psnr(self) -> float:
        """Over the three channels together."""
        return _psnr(sum(self.sse), 3 * self.samples)

    @property
    def max_abs(self) -> int:
        nz = np.nonzero(self.abs_hist.sum(axis=0))[0]
        return int(nz[-1]) if len(nz) else 0

    def count_beyond(self, k: int) -> int:
        """Samples (all channels) with |a - b| > k."""
        return int(self.abs_hist[:, max(0, int(k) + 1):].sum())

    def share_beyond(self, k: int) -> float:
        """The share of samples (all channels) with |a - b| > k."""
        n = 3 * self.samples
        return self.count_beyond(k) / n if n else 0.0

    @property
    def ssim_mean(self) -> float:
        return (self.ssim[0] + self.ssim[1] + self.ssim[2]) / 3.0

    def __eq__(self, other):
        if not isinstance(other, FrameMetrics):
            return NotImplemented
        return np.array_equal(self.abs_hist, other.abs_hist) and np.array(self.ssim).tobytes() == np.array(other.ssim).tobytes()

    def __repr__(self):
        return f"FrameMetrics(psnr={self.psnr:.4f}, ssim={self.ssim_mean:.6f}, max_abs={self.max_abs})"


def _check_call(n_frames: int, H: int, W: int, d_a: DeviceBuffer, d_b: DeviceBuffer) -> None:
    if not 1 <= n_frames <= MAX_FRAMES:
        raise ValueError(f"n_frames must be 1..{MAX_FRAMES} (got {n_frames})")
    if H < 1 or W < 1 or H * W >= 1 << 32:
        raise ValueError(f"bad frame size {H} x {W}")
    need = n_frames * H * W * 3
    if d_a.nbytes < need or d_b.nbytes < need:
        raise ValueError(f"{n_frames} frames of {H} x {W} need {need} bytes each; the buffers hold {d_a.nbytes} and {d_b.nbytes}")


def frame_metrics_launch(ctx: Context, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, d_out: DeviceBuffer, *,
                         ssim: bool = True, stream=None) -> None:
    """Enqueue the comparison of n_frames frames on `stream`; d_out takes n_frames records of RECORD_BYTES (records_from_bytes reads
    them).  Nothing is downloaded and nothing waits."""
    _check_call(n_frames, H, W, d_a, d_b)
    if d_out.nbytes < n_frames * RECORD_BYTES:
        raise ValueError(f"{n_frames} records need {n_frames * RECORD_BYTES} bytes; the buffer holds {d_out.nbytes}")
    ctx._check(lib.avx_frame_metrics_u8(ctx._h, d_a.ptr, d_b.ptr, int(n_frames), int(H), int(W), 1 if ssim else 0, d_out.ptr, ctx._s(stream)))


def records_from_bytes(buf: np.ndarray, n_frames: int) -> List[FrameMetrics]:
    """n_frames downloaded records (uint8) -> FrameMetrics."""
    recs = np.frombuffer(np.ascontiguousarray(buf).tobytes()[: n_frames * RECORD_BYTES], dtype=_RECORD_DTYPE)
    return [FrameMetrics(r["abs_hist"], r["ssim"]) for r in recs]


def frame_metrics_device(ctx: Context, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, *, ssim: bool = True,
                         stream=None) -> List[FrameMetrics]:
    """Compare n_frames (1..16) contiguous H x W x 3 uint8 frames of d_a with those of d_b; downloads the records."""
    _check_call(n_frames, H, W, d_a, d_b)
    d_out = ctx.malloc(n_frames * RECORD_BYTES)
    try:
        frame_metrics_launch(ctx, d_a, d_b, n_frames, H, W, d_out, ssim=ssim, stream=stream)
        raw = ctx.download(d_out, (n_frames * RECORD_BYTES,), np.uint8, stream=stream)
    finally:
        d_out.free()
    return records_from_bytes(raw, n_frames)


def check_pair(a, b):
    """Two uint8 arrays of one shape, H x W x 3 or N x H x W x 3 -> contiguous 4-D arrays and whether a frame axis was given.
    ValueError naming both otherwise, before any device work."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError(f"frames are uint8 (got a: {a.dtype} {a.shape}, b: {b.dtype} {b.shape})")
    if a.shape != b.shape:
        raise ValueError(f"a and b differ in shape (a: {a.shape}, b: {b.shape})")
    if a.ndim not in (3, 4) or a.shape[-1] != 3 or 0 in a.shape:
        raise ValueError(f"expected H x W x 3 or N x H x W x 3 (got a: {a.shape}, b: {b.shape})")
    batched = a.ndim == 4
    if not batched:
        a, b = a[None], b[None]
    return np.ascontiguousarray(a), np.ascontiguousarray(b), batched


def frame_metrics(a, b, *, ssim: bool = True, ctx: Optional[Context] = None):
    """a, b: uint8 H x W x 3 -> FrameMetrics, or N x H x W x 3 -> a list of N; uploaded in chunks of at most 16 frames."""
    a, b, batched = check_pair(a, b)
    N, H, W = a.shape[:3]
    ctx = ctx or get_context()
    chunk = min(N, MAX_FRAMES)
    d_a, d_b = ctx.malloc(chunk * H * W * 3), ctx.malloc(chunk * H * W * 3)
    out: List[FrameMetrics] = []
    try:
        for i in range(0, N, chunk):
            n = min(chunk, N - i)
            ctx.upload(a[i : i + n], d_a)
            ctx.upload(b[i : i + n], d_b)
            out += frame_metrics_device(ctx, d_a, d_b, n, H, W, ssim=ssim)
    finally:
        d_a.free()
        d_b.free()
    return out if batched else out[0]
