"""Frame comparison on the device (csrc/metrics.hip): what two uint8 RGB frames differ by -- per channel the exact
histogram of absolute code differences (from which SSE, PSNR, the largest difference and the share of samples beyond +-k codes follow
on the host without rounding) and the mean SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid positions only; the form
skimage computes with gaussian_weights=True, use_sample_covariance=False).

frame_metrics_device works on frames that are on the device already; frame_metrics takes arrays.  python -m animal_vision_amd.compare
is the command built on them.

plane_metrics (csrc/plane_metrics.hip) is the same comparison of video payloads in their own Y, U and V planes, at 8 or
10 bits, without any conversion: PlaneMetrics, plane_metrics_launch, plane_metrics_device and plane_metrics are the counterparts of
the four above.

MsSsim (csrc/ms_ssim.hip) is MS-SSIM over five scales (Wang, Simoncelli, Bovik 2003) of the same RGB frames:
frame_metrics_ms_launch / frame_metrics_ms_device return it beside the FrameMetrics of the same call, ms_ssim takes arrays.

Difference maps (csrc/diff_map.hip) say where the frames differ: diff_map_launch enqueues the per-pixel map ("abs",
"heat" or "ssim"; alone or A | B | map side by side) and a DiffRecord per frame, diff_map and ssim_map take arrays.
python -m animal_vision_amd.diff is the command built on them.

Colour difference maps (csrc/delta_e.hip) say how far apart the frames are in perceptual units: CIEDE2000 in CIELAB per
pixel.  delta_e_launch enqueues the float32 values, the map ("heat" or "plain"; alone or A | B | map) and a DeltaE record per frame;
delta_e, delta_e_map and delta_e_values take arrays.  python -m animal_vision_amd.deltae is the command built on them.

S-CIELAB (csrc/scielab.hip) is the same difference for a viewer at a stated distance: both frames are filtered by the
eye's contrast sensitivity at `ppd` pixels per degree before dE00 is taken.  scielab_launch, scielab, scielab_map and scielab_values
are the counterparts of the four above and return the same DeltaE records; `deltae --ppd` is the command.

Receptor-noise-limited distance (csrc/receptor.hip; Vorobyev & Osorio 1998) asks the question of another observer: can an
animal with these receptor classes and these Weber fractions tell the two colours apart, and where.  An Observer is a K x 3 matrix on
linear RGB with K Weber fractions (observer_for builds the one of a dichromat species or of HoneyBee); receptor_delta_launch,
receptor_delta, receptor_delta_map and receptor_delta_values return dS in just-noticeable differences in the same DeltaE records, maps
and value planes; `deltae --observer` is the command.  With acuity=SIGMA (csrc/receptor_acuity.hip) both frames are first
blurred in linear light by the observer's acuity, a Gaussian of SIGMA pixels -- species_acuity gives the one a species' own rendering
uses --, so that what the animal cannot resolve counts for little; `deltae --acuity` is the command.

dE_ITP (csrc/itp.hip; ITU-R BT.2124) is the colour difference that is defined at HDR light levels: 720 x the distance in
ICtCp with Ct halved.  A side is an HdrFrames (10-bit PQ or HLG payloads as stored) or a uint8 sRGB array shown at sdr_white nits, in
any mix; itp_delta_launch, itp_delta, itp_delta_map and itp_delta_values return the same DeltaE records, maps and value planes;
`deltae --itp` is the command.

Receptor contrast within a frame (csrc/receptor_edges.hip; Local Edge Intensity Analysis, van den Berg et al. 2020) takes
one input: per pixel the largest receptor-noise-limited contrast to its up to eight neighbours `step` pixels away, behind the acuity
blur -- chromatic, achromatic (a luminance channel: achromatic=(classes, weber)) or either.  receptor_edges_launch, receptor_edges,
receptor_edges_map and receptor_edges_values return the same DeltaE records, maps and value planes; smooth=(radius, keep[, iterations])
puts the edge-preserving smoothing of csrc/receptor_smooth.hip in front of the edges and receptor_smooth_planes returns the
smoothed planes; python -m animal_vision_amd.edges is the command."""
from __future__ import annotations

import ctypes
import dataclasses
import math
import numbers
from typing import List, Optional, Tuple

import numpy as np

from ._lib import AVX_DELTA_E_LAYOUTS, AVX_DELTA_E_MODES, AVX_DIFF_LAYOUTS, AVX_DIFF_MODES, AVX_METRICS_MAX_FRAMES, AVX_PIX_FMTS, FrameMetricsRecord, MsSsimRecord, PlaneMetricsRecord, lib
from ._lib import DeltaERecord as DeltaERecordStruct
from ._lib import DiffRecord as DiffRecordStruct
from ._lib import ItpSide as ItpSideStruct
from ._lib import AVX_EDGES_CHANNELS, LuminanceDesc, ReceptorDesc, SmoothDesc
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


def _records(buf: np.ndarray, n: int, nbytes: int, dtype: np.dtype) -> np.ndarray:
    """The first n records of `nbytes` each in a downloaded uint8 buffer, as a structured array (a copy)."""
    return np.frombuffer(np.ascontiguousarray(buf).tobytes()[: n * nbytes], dtype=dtype)


def _walk(ctx: Optional[Context], a: np.ndarray, b: np.ndarray, per_chunk, extra=()) -> None:
    """The array-level entry points' loop: a and b (N frames or payloads each) go up in chunks of at most MAX_FRAMES, and
    per_chunk(ctx, i, n, d_a, d_b, *d_extra) works on the n frames from frame i on.  The device buffers hold min(N, MAX_FRAMES)
    frames; `extra` names further ones in bytes per frame (None: no buffer, None is passed).  All are freed however it ends."""
    ctx = ctx or get_context()
    N = len(a)
    chunk = min(N, MAX_FRAMES)
    bufs: List[Optional[DeviceBuffer]] = []
    try:
        for nbytes in (a[0].nbytes, b[0].nbytes, *extra):
            bufs.append(None if nbytes is None else ctx.malloc(chunk * nbytes))
        for i in range(0, N, chunk):
            n = min(chunk, N - i)
            ctx.upload(a[i : i + n], bufs[0])
            ctx.upload(b[i : i + n], bufs[1])
            per_chunk(ctx, i, n, *bufs)
    finally:
        for d in bufs:
            if d is not None:
                d.free()


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
    return [FrameMetrics(r["abs_hist"], r["ssim"]) for r in _records(buf, n_frames, RECORD_BYTES, _RECORD_DTYPE)]


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
    H, W = a.shape[1:3]
    out: List[FrameMetrics] = []
    _walk(ctx, a, b, lambda ctx, i, n, d_a, d_b: out.extend(frame_metrics_device(ctx, d_a, d_b, n, H, W, ssim=ssim)))
    return out if batched else out[0]


# ------------------------------------------------------------------------------------------------ YUV planes
PLANE_RECORD_BYTES = ctypes.sizeof(PlaneMetricsRecord)  # 3 * 1024 uint32, then 3 doubles
_PLANE_DTYPE = np.dtype([("abs_hist", np.uint32, (3, 1024)), ("ssim", np.float64, (3,))])
assert _PLANE_DTYPE.itemsize == PLANE_RECORD_BYTES
# pix_fmt: (log2 horizontal chroma subsampling, log2 vertical, sample depth, luma only) -- csrc/yuv_formats.h
_PLANE_FORMATS = {"yuv420p": (1, 1, 8, False), "nv12": (1, 1, 8, False), "yuv422p": (1, 0, 8, False), "yuv444p": (0, 0, 8, False),
                  "gray": (0, 0, 8, True), "yuv420p10le": (1, 1, 10, False), "yuv422p10le": (1, 0, 10, False),
                  "yuv444p10le": (0, 0, 10, False), "p010le": (1, 1, 10, False)}
assert set(_PLANE_FORMATS) == set(AVX_PIX_FMTS)


def plane_geometry(pix_fmt: str, H: int, W: int):
    """(depth, (Y, U, V sample counts)) of one H x W frame in `pix_fmt`; absent planes count 0."""
    if pix_fmt not in _PLANE_FORMATS:
        raise ValueError(f"pix_fmt must be one of {', '.join(_PLANE_FORMATS)} (got {pix_fmt!r})")
    sx, sy, depth, luma = _PLANE_FORMATS[pix_fmt]
    c = 0 if luma else (-(-H >> sy)) * (-(-W >> sx))
    return depth, (H * W, c, c)


def check_plane_formats(pix_fmt: str, pix_fmt_b: Optional[str] = None) -> str:
    """The format of B (pix_fmt when None); ValueError when the two disagree in sample depth or chroma subsampling."""
    pix_fmt_b = pix_fmt if pix_fmt_b is None else pix_fmt_b
    for f in (pix_fmt, pix_fmt_b):
        if f not in _PLANE_FORMATS:
            raise ValueError(f"pix_fmt must be one of {', '.join(_PLANE_FORMATS)} (got {f!r})")
    if _PLANE_FORMATS[pix_fmt] != _PLANE_FORMATS[pix_fmt_b]:
        raise ValueError(f"{pix_fmt} and {pix_fmt_b} disagree in sample depth or chroma subsampling: planes are compared as stored")
    return pix_fmt_b


class PlaneMetrics:
    """One frame's record in YUV planes: abs_hist[p][k] = samples of plane p (Y, U, V) with |a - b| == k in native codes (3 x bins
    uint64, bins = 2^depth), ssim[p] = mean SSIM of plane p (NaN where it was not computed or the plane is absent), plane_samples =
    the planes' sample counts, planes = "yuv" or "y".  Everything else is derived from the histogram, in integers where it is a
    count."""

    __slots__ = ("abs_hist", "ssim", "depth", "plane_samples", "planes")

    def __init__(self, abs_hist, ssim=(math.nan, math.nan, math.nan), depth: int = 8, plane_samples=None):
        if depth not in (8, 10):
            raise ValueError(f"depth is 8 or 10 (got {depth})")
        h = np.asarray(abs_hist)
        if h.ndim != 2 or h.shape[0] != 3 or h.shape[1] < (1 << depth) or h[:, 1 << depth:].any():
            raise ValueError(f"abs_hist is 3 x {1 << depth} at {depth} bits (got {h.shape})")
        self.abs_hist = h[:, : 1 << depth].astype(np.uint64)
        self.ssim = tuple(float(v) for v in ssim)
        if len(self.ssim) != 3:
            raise ValueError(f"ssim holds three values (got {len(self.ssim)})")
        self.depth = int(depth)
        sums = tuple(int(v) for v in self.abs_hist.sum(axis=1))
        self.plane_samples = sums if plane_samples is None else tuple(int(v) for v in plane_samples)
        if self.plane_samples != sums:
            raise ValueError(f"the histogram rows sum to {sums}, the planes hold {self.plane_samples} samples")
        self.planes = "yuv" if self.plane_samples[1] or self.plane_samples[2] else "y"

    @property
    def peak(self) -> int:
        return (1 << self.depth) - 1

    @property
    def samples(self) -> int:
        """Samples of all planes together."""
        return sum(self.plane_samples)

    @property
    def sse(self) -> tuple:
        """Per plane: the sum of squared differences, sum_k k^2 * hist[p][k]."""
        k2 = np.arange(1 << self.depth, dtype=np.uint64) ** 2
        return tuple(int((self.abs_hist[p] * k2).sum()) for p in range(3))

    def _psnr(self, sse: int, n: int) -> float:
        if n == 0:
            return math.nan
        return math.inf if sse == 0 else 10.0 * math.log10(float(self.peak) ** 2 * n / sse)

    @property
    def psnr_planes(self) -> tuple:
        """Per plane: 10 log10(peak^2 N_p / SSE_p), inf at SSE = 0, NaN for an absent plane."""
        return tuple(self._psnr(s, n) for s, n in zip(self.sse, self.plane_samples))

    @property
    def psnr(self) -> float:
        """Pooled over all samples of all planes (ffmpeg's `average`)."""
        return self._psnr(sum(self.sse), self.samples)

    @property
    def max_abs(self) -> int:
        nz = np.nonzero(self.abs_hist.sum(axis=0))[0]
        return int(nz[-1]) if len(nz) else 0

    def count_beyond(self, k: int) -> int:
        """Samples (all planes) with |a - b| > k native codes."""
        return int(self.abs_hist[:, max(0, int(k) + 1):].sum())

    def share_beyond(self, k: int) -> float:
        n = self.samples
        return self.count_beyond(k) / n if n else 0.0

    @property
    def ssim_mean(self) -> float:
        """The planes' SSIM weighted by their sample counts ((4 Y + U + V) / 6 at 4:2:0); NaN planes are left out."""
        num = den = 0.0
        for v, n in zip(self.ssim, self.plane_samples):
            if not math.isnan(v) and n:
                num, den = num + v * n, den + n
        return num / den if den else math.nan

    def __eq__(self, other):
        if not isinstance(other, PlaneMetrics):
            return NotImplemented
        return (self.depth == other.depth and np.array_equal(self.abs_hist, other.abs_hist)
                and np.array(self.ssim).tobytes() == np.array(other.ssim).tobytes())

    def __repr__(self):
        return f"PlaneMetrics({self.depth}-bit {self.planes}, psnr={self.psnr:.4f}, ssim={self.ssim_mean:.6f}, max_abs={self.max_abs})"


def _check_plane_call(pix_fmt: str, pix_fmt_b: str, n_frames: int, H: int, W: int, d_a: DeviceBuffer, d_b: DeviceBuffer):
    from .yuv import frame_size

    check_plane_formats(pix_fmt, pix_fmt_b)
    if not 1 <= n_frames <= MAX_FRAMES:
        raise ValueError(f"n_frames must be 1..{MAX_FRAMES} (got {n_frames})")
    if H < 1 or W < 1:
        raise ValueError(f"bad frame size {H} x {W}")
    need_a, need_b = n_frames * frame_size(pix_fmt, H, W), n_frames * frame_size(pix_fmt_b, H, W)
    if d_a.nbytes < need_a or d_b.nbytes < need_b:
        raise ValueError(f"{n_frames} frames of {H} x {W} need {need_a} ({pix_fmt}) and {need_b} ({pix_fmt_b}) bytes; the buffers hold "
                         f"{d_a.nbytes} and {d_b.nbytes}")


def plane_metrics_launch(ctx: Context, pix_fmt: str, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, d_out: DeviceBuffer,
                         *, pix_fmt_b: Optional[str] = None, ssim: bool = True, stream=None) -> None:
    """Enqueue the comparison of n_frames payloads on `stream`; d_out takes n_frames records of PLANE_RECORD_BYTES
    (plane_records_from_bytes reads them).  Nothing is downloaded and nothing waits."""
    pix_fmt_b = pix_fmt if pix_fmt_b is None else pix_fmt_b
    _check_plane_call(pix_fmt, pix_fmt_b, n_frames, H, W, d_a, d_b)
    if d_out.nbytes < n_frames * PLANE_RECORD_BYTES:
        raise ValueError(f"{n_frames} records need {n_frames * PLANE_RECORD_BYTES} bytes; the buffer holds {d_out.nbytes}")
    ctx._check(lib.avx_plane_metrics(ctx._h, AVX_PIX_FMTS[pix_fmt], d_a.ptr, AVX_PIX_FMTS[pix_fmt_b], d_b.ptr, int(n_frames), int(H), int(W),
                                     1 if ssim else 0, d_out.ptr, ctx._s(stream)))


def plane_records_from_bytes(buf: np.ndarray, n_frames: int, pix_fmt: str, H: int, W: int) -> List[PlaneMetrics]:
    """n_frames downloaded records (uint8) of H x W frames in `pix_fmt` -> PlaneMetrics."""
    depth, counts = plane_geometry(pix_fmt, H, W)
    return [PlaneMetrics(r["abs_hist"], r["ssim"], depth, counts) for r in _records(buf, n_frames, PLANE_RECORD_BYTES, _PLANE_DTYPE)]


def plane_metrics_device(ctx: Context, pix_fmt: str, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, *,
                         pix_fmt_b: Optional[str] = None, ssim: bool = True, stream=None) -> List[PlaneMetrics]:
    """Compare n_frames (1..16) contiguous payloads of d_a (pix_fmt) with those of d_b (pix_fmt_b); downloads the records."""
    pix_fmt_b = pix_fmt if pix_fmt_b is None else pix_fmt_b
    _check_plane_call(pix_fmt, pix_fmt_b, n_frames, H, W, d_a, d_b)
    d_out = ctx.malloc(n_frames * PLANE_RECORD_BYTES)
    try:
        plane_metrics_launch(ctx, pix_fmt, d_a, d_b, n_frames, H, W, d_out, pix_fmt_b=pix_fmt_b, ssim=ssim, stream=stream)
        raw = ctx.download(d_out, (n_frames * PLANE_RECORD_BYTES,), np.uint8, stream=stream)
    finally:
        d_out.free()
    return plane_records_from_bytes(raw, n_frames, pix_fmt, H, W)


def check_payloads(a, b, pix_fmt: str, pix_fmt_b: str, H: int, W: int):
    """Two uint8 payload arrays (n x frame_size, or one flat payload each) -> contiguous 2-D arrays.  ValueError naming both
    otherwise, before any device work."""
    from .yuv import frame_size

    check_plane_formats(pix_fmt, pix_fmt_b)
    if H < 1 or W < 1:
        raise ValueError(f"bad frame size {H} x {W}")
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError(f"payloads are uint8 (got a: {a.dtype} {a.shape}, b: {b.dtype} {b.shape})")
    sa, sb = frame_size(pix_fmt, H, W), frame_size(pix_fmt_b, H, W)
    if a.ndim not in (1, 2) or b.ndim not in (1, 2) or a.shape[-1] != sa or b.shape[-1] != sb:
        raise ValueError(f"a {H} x {W} frame is {sa} bytes of {pix_fmt} and {sb} bytes of {pix_fmt_b} (got a: {a.shape}, b: {b.shape})")
    a, b = a.reshape(-1, sa), b.reshape(-1, sb)
    if len(a) != len(b) or len(a) == 0:
        raise ValueError(f"a and b differ in length, or are empty (a: {len(a)} frames, b: {len(b)} frames)")
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def plane_metrics(a, b, *, pix_fmt: str, H: int, W: int, pix_fmt_b: Optional[str] = None, ssim: bool = True,
                  ctx: Optional[Context] = None) -> List[PlaneMetrics]:
    """a, b: uint8 payloads of H x W frames (n x frame_size, or one flat payload) in pix_fmt and pix_fmt_b (default: pix_fmt) -> a
    list of n PlaneMetrics; uploaded in chunks of at most 16 frames."""
    pix_fmt_b = pix_fmt if pix_fmt_b is None else pix_fmt_b
    a, b = check_payloads(a, b, pix_fmt, pix_fmt_b, int(H), int(W))
    out: List[PlaneMetrics] = []
    _walk(ctx, a, b, lambda ctx, i, n, d_a, d_b: out.extend(plane_metrics_device(ctx, pix_fmt, d_a, d_b, n, H, W, pix_fmt_b=pix_fmt_b, ssim=ssim)))
    return out


# ------------------------------------------------------------------------------------------------ MS-SSIM
MS_RECORD_BYTES = ctypes.sizeof(MsSsimRecord)  # cs[3][5], ssim[3][5]: 30 doubles
_MS_DTYPE = np.dtype([("cs", np.float64, (3, 5)), ("ssim", np.float64, (3, 5))])
assert _MS_DTYPE.itemsize == MS_RECORD_BYTES == 240
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)  # Wang, Simoncelli, Bovik 2003, scales 0..4
MS_MIN_SIDE = 176  # scale 4 is floor(H / 16) x floor(W / 16) and needs one 11 x 11 window position


class MsSsim:
    """One frame's per-scale means: cs[c][j] = mean contrast-structure term of channel c at scale j, ssim[c][j] = mean SSIM there
    (3 x 5 float64 each, as the device wrote them: not clamped).  The product over the scales is formed here, in float64."""

    __slots__ = ("cs", "ssim")

    def __init__(self, cs, ssim):
        self.cs, self.ssim = np.array(cs, dtype=np.float64), np.array(ssim, dtype=np.float64)
        if self.cs.shape != (3, 5) or self.ssim.shape != (3, 5):
            raise ValueError(f"cs and ssim are 3 x 5 (got {self.cs.shape} and {self.ssim.shape})")

    @property
    def ms_ssim_channels(self) -> tuple:
        """Per channel: prod_{j<4} max(cs[j], 0)^w_j * max(ssim[4], 0)^w_4 (the clamp is TensorFlow's and pytorch-msssim's)."""
        out = []
        for c in range(3):
            v = max(float(self.ssim[c][4]), 0.0) ** MS_WEIGHTS[4]
            for j in range(4):
                v *= max(float(self.cs[c][j]), 0.0) ** MS_WEIGHTS[j]
            out.append(v)
        return tuple(out)

    @property
    def ms_ssim(self) -> float:
        """The mean of the three channels."""
        v = self.ms_ssim_channels
        return (v[0] + v[1] + v[2]) / 3.0

    def __eq__(self, other):
        if not isinstance(other, MsSsim):
            return NotImplemented
        return self.cs.tobytes() == other.cs.tobytes() and self.ssim.tobytes() == other.ssim.tobytes()

    def __repr__(self):
        return f"MsSsim(ms_ssim={self.ms_ssim:.6f})"


def check_ms_size(H: int, W: int) -> None:
    """ValueError for a frame too small for five scales."""
    if H < MS_MIN_SIDE or W < MS_MIN_SIDE:
        raise ValueError(f"MS-SSIM over five scales needs frames of at least {MS_MIN_SIDE} x {MS_MIN_SIDE} (got {H} x {W})")


def frame_metrics_ms_launch(ctx: Context, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, d_out: DeviceBuffer,
                            d_ms: DeviceBuffer, *, stream=None) -> None:
    """Enqueue the comparison with MS-SSIM of n_frames frames on `stream`; d_out takes n_frames records of RECORD_BYTES (the bytes
    frame_metrics_launch writes), d_ms n_frames of MS_RECORD_BYTES (ms_records_from_bytes reads them).  Nothing is downloaded and
    nothing waits."""
    _check_call(n_frames, H, W, d_a, d_b)
    check_ms_size(H, W)
    if d_out.nbytes < n_frames * RECORD_BYTES or d_ms.nbytes < n_frames * MS_RECORD_BYTES:
        raise ValueError(f"{n_frames} records need {n_frames * RECORD_BYTES} and {n_frames * MS_RECORD_BYTES} bytes; the buffers hold "
                         f"{d_out.nbytes} and {d_ms.nbytes}")
    ctx._check(lib.avx_frame_metrics_ms_u8(ctx._h, d_a.ptr, d_b.ptr, int(n_frames), int(H), int(W), d_out.ptr, d_ms.ptr, ctx._s(stream)))


def ms_records_from_bytes(buf: np.ndarray, n_frames: int) -> List[MsSsim]:
    """n_frames downloaded MS-SSIM records (uint8) -> MsSsim."""
    return [MsSsim(r["cs"], r["ssim"]) for r in _records(buf, n_frames, MS_RECORD_BYTES, _MS_DTYPE)]


def frame_metrics_ms_device(ctx: Context, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, *, stream=None):
    """Compare n_frames (1..16) contiguous H x W x 3 uint8 frames of d_a with those of d_b; downloads both kinds of records:
    (list of FrameMetrics, list of MsSsim)."""
    _check_call(n_frames, H, W, d_a, d_b)
    check_ms_size(H, W)
    d_out, d_ms = ctx.malloc(n_frames * RECORD_BYTES), ctx.malloc(n_frames * MS_RECORD_BYTES)
    try:
        frame_metrics_ms_launch(ctx, d_a, d_b, n_frames, H, W, d_out, d_ms, stream=stream)
        raw = ctx.download(d_out, (n_frames * RECORD_BYTES,), np.uint8, stream=stream)
        raw_ms = ctx.download(d_ms, (n_frames * MS_RECORD_BYTES,), np.uint8, stream=stream)
    finally:
        d_out.free()
        d_ms.free()
    return records_from_bytes(raw, n_frames), ms_records_from_bytes(raw_ms, n_frames)


def ms_ssim(a, b, *, ctx: Optional[Context] = None):
    """a, b: uint8 H x W x 3 -> MsSsim, or N x H x W x 3 -> a list of N; uploaded in chunks of at most 16 frames.  ValueError for
    frames below 176 x 176, before any device work."""
    a, b, batched = check_pair(a, b)
    H, W = a.shape[1:3]
    check_ms_size(H, W)
    out: List[MsSsim] = []
    _walk(ctx, a, b, lambda ctx, i, n, d_a, d_b: out.extend(frame_metrics_ms_device(ctx, d_a, d_b, n, H, W)[1]))
    return out if batched else out[0]


# ------------------------------------------------------------------------------------------------ difference maps
DIFF_RECORD_BYTES = ctypes.sizeof(DiffRecordStruct)  # max_d, max_x, max_y, beyond: 4 uint32
_DIFF_DTYPE = np.dtype([("max_d", np.uint32), ("max_x", np.uint32), ("max_y", np.uint32), ("beyond", np.uint32)])
assert _DIFF_DTYPE.itemsize == DIFF_RECORD_BYTES == 16
DIFF_MODES, DIFF_LAYOUTS = tuple(AVX_DIFF_MODES), tuple(AVX_DIFF_LAYOUTS)
DIFF_DEFAULT_GAIN = {"abs": 32, "heat": 32, "ssim": 4.0}
SSIM_WINDOW = 11  # the SSIM mode needs one window position: frames of at least 11 x 11


class DiffRecord:
    """One frame's record of a difference map: max_d = the largest d = max_c |a_c - b_c| of the frame, (max_x, max_y) = the first
    pixel in raster order that attains it ((0, 0) when max_d is 0), beyond = the number of pixels with d above the threshold."""

    __slots__ = ("max_d", "max_x", "max_y", "beyond")

    def __init__(self, max_d: int, max_x: int, max_y: int, beyond: int):
        self.max_d, self.max_x, self.max_y, self.beyond = int(max_d), int(max_x), int(max_y), int(beyond)

    def astuple(self) -> tuple:
        return self.max_d, self.max_x, self.max_y, self.beyond

    def __eq__(self, other):
        if not isinstance(other, DiffRecord):
            return NotImplemented
        return self.astuple() == other.astuple()

    def __repr__(self):
        return f"DiffRecord(max_d={self.max_d}, at=({self.max_x}, {self.max_y}), beyond={self.beyond})"


def check_diff_options(mode: str, gain, threshold, layout: str, H: Optional[int] = None, W: Optional[int] = None):
    """The gain (the mode's default when None) as the number the library takes, after the checks of avx_diff_map_u8 that need no
    device; ValueError naming the option otherwise."""
    if mode not in AVX_DIFF_MODES:
        raise ValueError(f"mode must be one of {', '.join(AVX_DIFF_MODES)} (got {mode!r})")
    if layout not in AVX_DIFF_LAYOUTS:
        raise ValueError(f"layout must be one of {', '.join(AVX_DIFF_LAYOUTS)} (got {layout!r})")
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Integral) or not 0 <= threshold <= 254:
        raise ValueError(f"threshold must be an integer 0..254 (got {threshold!r})")
    gain = DIFF_DEFAULT_GAIN[mode] if gain is None else gain
    if mode == "ssim":
        if not (isinstance(gain, numbers.Real) and 0.0 < gain <= 16.0):
            raise ValueError(f"the gain of mode ssim must be above 0 and at most 16 (got {gain!r})")
        if H is not None and W is not None and (H < SSIM_WINDOW or W < SSIM_WINDOW):
            raise ValueError(f"mode ssim needs frames of at least {SSIM_WINDOW} x {SSIM_WINDOW} (got {H} x {W})")
    elif not (isinstance(gain, numbers.Real) and float(gain).is_integer() and 1 <= gain <= 255):
        raise ValueError(f"the gain of mode {mode} must be an integer 1..255 (got {gain!r})")
    return float(gain)


def diff_map_launch(ctx: Context, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, d_out: DeviceBuffer, d_rec: DeviceBuffer,
                    *, mode: str = "heat", gain=None, threshold: int = 1, layout: str = "map", d_ssim_map: Optional[DeviceBuffer] = None,
                    stream=None) -> None:
    """Enqueue the difference maps of n_frames frames on `stream`: d_out takes n_frames frames of H x W x 3 (layout "map") or
    H x 3W x 3 ("side": A | B | map), d_rec n_frames records of DIFF_RECORD_BYTES (diff_records_from_bytes reads them), d_ssim_map
    (mode "ssim" only) the float32 SSIM of every window position, n_frames x (H - 10) x (W - 10) x 3.  Nothing is downloaded and
    nothing waits."""
    _check_call(n_frames, H, W, d_a, d_b)
    g = check_diff_options(mode, gain, threshold, layout, H, W)
    need = n_frames * H * W * 3 * (3 if layout == "side" else 1)
    if d_out.nbytes < need or d_rec.nbytes < n_frames * DIFF_RECORD_BYTES:
        raise ValueError(f"{n_frames} {layout} frames and records need {need} and {n_frames * DIFF_RECORD_BYTES} bytes; the buffers hold "
                         f"{d_out.nbytes} and {d_rec.nbytes}")
    if d_ssim_map is not None:
        if mode != "ssim":
            raise ValueError(f"d_ssim_map goes with mode ssim only (got mode {mode!r})")
        need = n_frames * (H - 10) * (W - 10) * 3 * 4
        if d_ssim_map.nbytes < need:
            raise ValueError(f"the SSIM of {n_frames} frames' positions needs {need} bytes; the buffer holds {d_ssim_map.nbytes}")
    ctx._check(lib.avx_diff_map_u8(ctx._h, d_a.ptr, d_b.ptr, int(n_frames), int(H), int(W), AVX_DIFF_MODES[mode], g, int(threshold),
                                   AVX_DIFF_LAYOUTS[layout], d_out.ptr, d_rec.ptr, None if d_ssim_map is None else d_ssim_map.ptr, ctx._s(stream)))


def diff_records_from_bytes(buf: np.ndarray, n_frames: int) -> List[DiffRecord]:
    """n_frames downloaded records (uint8) -> DiffRecord."""
    return [DiffRecord(r["max_d"], r["max_x"], r["max_y"], r["beyond"]) for r in _records(buf, n_frames, DIFF_RECORD_BYTES, _DIFF_DTYPE)]


def _diff_chunks(a, b, mode, gain, threshold, layout, ctx, with_float):
    """diff_map and ssim_map: the stack in chunks of at most 16 frames -> (frames, records, float maps or None)."""
    N, H, W = a.shape[:3]
    wide = 3 if layout == "side" else 1
    frames, recs = np.empty((N, H, W * wide, 3), np.uint8), []
    maps = np.empty((N, H - 10, W - 10, 3), np.float32) if with_float else None

    def per_chunk(ctx, i, n, d_a, d_b, d_out, d_rec, d_map):
        diff_map_launch(ctx, d_a, d_b, n, H, W, d_out, d_rec, mode=mode, gain=gain, threshold=threshold, layout=layout, d_ssim_map=d_map)
        ctx.download(d_out, (n, H, W * wide, 3), np.uint8, out=frames[i : i + n])
        recs.extend(diff_records_from_bytes(ctx.download(d_rec, (n * DIFF_RECORD_BYTES,), np.uint8), n))
        if with_float:
            ctx.download(d_map, (n, H - 10, W - 10, 3), np.float32, out=maps[i : i + n])

    _walk(ctx, a, b, per_chunk, (H * W * 3 * wide, DIFF_RECORD_BYTES, (H - 10) * (W - 10) * 12 if with_float else None))
    return frames, recs, maps


def diff_map(a, b, *, mode: str = "heat", gain=None, threshold: int = 1, layout: str = "map", ctx: Optional[Context] = None):
    """a, b: uint8 H x W x 3 -> (the map, uint8 H x W x 3 -- H x 3W x 3 with layout "side" --, its DiffRecord), or N x H x W x 3 ->
    (N maps, a list of N records); uploaded in chunks of at most 16 frames.  mode: "abs", "heat" or "ssim"; gain: the mode's
    default (32, 32, 4) when None.  ValueError for a bad option or shape before any device work."""
    a, b, batched = check_pair(a, b)
    check_diff_options(mode, gain, threshold, layout, a.shape[1], a.shape[2])
    frames, recs, _ = _diff_chunks(a, b, mode, gain, threshold, layout, ctx, False)
    return (frames, recs) if batched else (frames[0], recs[0])


def ssim_map(a, b, *, ctx: Optional[Context] = None) -> np.ndarray:
    """a, b: uint8 H x W x 3 or N x H x W x 3 (at least 11 x 11) -> the SSIM of every window position and channel as the map kernel
    forms it, float32 N x (H - 10) x (W - 10) x 3 (N = 1 for one frame): the values whose mean is FrameMetrics.ssim."""
    a, b, _ = check_pair(a, b)
    check_diff_options("ssim", None, 1, "map", a.shape[1], a.shape[2])
    return _diff_chunks(a, b, "ssim", None, 1, "map", ctx, True)[2]


# ------------------------------------------------------------------------------------------------ colour difference maps
DELTA_E_RECORD_BYTES = ctypes.sizeof(DeltaERecordStruct)  # hist[256] uint32, sum double, max_de float, max_x, max_y, beyond uint32
_DELTA_E_DTYPE = np.dtype([("hist", np.uint32, (256,)), ("sum", np.float64), ("max_de", np.float32), ("max_x", np.uint32), ("max_y", np.uint32),
                           ("beyond", np.uint32)])
assert _DELTA_E_DTYPE.itemsize == DELTA_E_RECORD_BYTES == 1048
DELTA_E_MODES, DELTA_E_LAYOUTS = tuple(AVX_DELTA_E_MODES), tuple(AVX_DELTA_E_LAYOUTS)
DELTA_E_DEFAULT_GAIN = 10.0
DELTA_E_DEFAULT_THRESHOLD = 1.0  # about one just-noticeable difference


class DeltaE:
    """One frame's record of a colour difference map: hist[k] = pixels with min(255, floor(2 dE)) == k (bins 0.5 wide, the last one
    open), sum = the float64 sum of the pixels' float32 dE, max_de = the largest with (max_x, max_y) the first pixel in raster order
    that attains it ((0, 0) when it is 0), beyond = pixels with dE above the threshold.  mean and percentile follow here."""

    __slots__ = ("hist", "sum", "max_de", "max_x", "max_y", "beyond")

    def __init__(self, hist, sum, max_de, max_x, max_y, beyond):  # noqa: A002  (the record's field is called sum)
        h = np.asarray(hist)
        if h.shape != (256,):
            raise ValueError(f"hist holds 256 bins (got {h.shape})")
        self.hist = h.astype(np.uint64)
        self.sum, self.max_de = float(sum), float(max_de)
        self.max_x, self.max_y, self.beyond = int(max_x), int(max_y), int(beyond)

    @property
    def pixels(self) -> int:
        """H * W."""
        return int(self.hist.sum())

    @property
    def mean(self) -> float:
        n = self.pixels
        return self.sum / n if n else 0.0

    def percentile(self, q: float) -> float:
        """The upper edge (k + 1) / 2 of the first bin k whose cumulative count reaches ceil(q H W), 0 < q <= 1; where that is the
        open last bin, max_de."""
        if not 0.0 < q <= 1.0:
            raise ValueError(f"q must be above 0 and at most 1 (got {q!r})")
        need = math.ceil(q * self.pixels)
        k = int(np.searchsorted(np.cumsum(self.hist), need, side="left"))
        return self.max_de if k >= 255 else (k + 1) / 2.0

    def _key(self):
        return self.hist.tobytes(), np.float64(self.sum).tobytes(), np.float32(self.max_de).tobytes(), self.max_x, self.max_y, self.beyond

    def __eq__(self, other):
        if not isinstance(other, DeltaE):
            return NotImplemented
        return self._key() == other._key()

    def __repr__(self):
        return f"DeltaE(mean={self.mean:.4f}, max_de={self.max_de:.4f}, at=({self.max_x}, {self.max_y}), beyond={self.beyond})"


def check_delta_e_options(mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD, layout: str = "map"):
    """(gain, threshold) as the numbers the library takes -- the default gain (10) when None -- after the checks of avx_delta_e_u8
    that need no device; ValueError naming the option otherwise."""
    if mode not in AVX_DELTA_E_MODES:
        raise ValueError(f"mode must be one of {', '.join(AVX_DELTA_E_MODES)} (got {mode!r})")
    if layout not in AVX_DELTA_E_LAYOUTS:
        raise ValueError(f"layout must be one of {', '.join(AVX_DELTA_E_LAYOUTS)} (got {layout!r})")
    gain = DELTA_E_DEFAULT_GAIN if gain is None else gain
    if isinstance(gain, bool) or not isinstance(gain, numbers.Real) or not (math.isfinite(gain) and 0.0 < gain <= 255.0):
        raise ValueError(f"gain must be above 0 and at most 255 (got {gain!r})")
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or not (math.isfinite(threshold) and threshold >= 0.0):
        raise ValueError(f"threshold must be finite and at least 0 (got {threshold!r})")
    return float(gain), float(threshold)


def _check_delta_e_buffers(n_frames: int, H: int, W: int, d_map, d_rec, d_float, mode, gain, threshold, layout):
    """check_delta_e_options, then the sizes of the buffers a colour difference launch writes; (gain, threshold) as floats."""
    g, t = check_delta_e_options(mode, gain, threshold, layout)
    if d_rec.nbytes < n_frames * DELTA_E_RECORD_BYTES:
        raise ValueError(f"{n_frames} records need {n_frames * DELTA_E_RECORD_BYTES} bytes; the buffer holds {d_rec.nbytes}")
    need = n_frames * H * W * 3 * (3 if layout == "side" else 1)
    if d_map is not None and d_map.nbytes < need:
        raise ValueError(f"{n_frames} {layout} frames need {need} bytes; the buffer holds {d_map.nbytes}")
    if d_float is not None and d_float.nbytes < n_frames * H * W * 4:
        raise ValueError(f"the values of {n_frames} frames need {n_frames * H * W * 4} bytes; the buffer holds {d_float.nbytes}")
    return g, t


def delta_e_launch(ctx: Context, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, d_map: Optional[DeviceBuffer],
                   d_rec: DeviceBuffer, *, mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD, layout: str = "map",
                   d_float: Optional[DeviceBuffer] = None, stream=None) -> None:
    """Enqueue the colour difference of n_frames frames on `stream`: d_rec takes n_frames records of DELTA_E_RECORD_BYTES
    (delta_e_records_from_bytes reads them); d_map, when not None, n_frames frames of H x W x 3 (layout "map") or H x 3W x 3 ("side":
    A | B | map); d_float, when not None, the float32 dE of every pixel, n_frames x H x W.  Nothing is downloaded and nothing waits."""
    _check_call(n_frames, H, W, d_a, d_b)
    g, t = _check_delta_e_buffers(n_frames, H, W, d_map, d_rec, d_float, mode, gain, threshold, layout)
    ctx._check(lib.avx_delta_e_u8(ctx._h, d_a.ptr, d_b.ptr, int(n_frames), int(H), int(W), AVX_DELTA_E_MODES[mode], g, t, AVX_DELTA_E_LAYOUTS[layout],
                                  None if d_map is None else d_map.ptr, d_rec.ptr, None if d_float is None else d_float.ptr, ctx._s(stream)))


def delta_e_records_from_bytes(buf: np.ndarray, n_frames: int) -> List[DeltaE]:
    """n_frames downloaded records (uint8) -> DeltaE."""
    return [DeltaE(r["hist"], r["sum"], r["max_de"], r["max_x"], r["max_y"], r["beyond"])
            for r in _records(buf, n_frames, DELTA_E_RECORD_BYTES, _DELTA_E_DTYPE)]


def _delta_e_chunks(a, b, mode, gain, threshold, layout, ctx, with_map, with_float, ppd=None, observer=None, acuity=None):
    """delta_e, delta_e_map, delta_e_values and their scielab (with ppd) and receptor_delta (with observer) counterparts: the stack in
    chunks of at most 16 frames -> (maps or None, records, values or None)."""
    N, H, W = a.shape[:3]
    wide = 3 if layout == "side" else 1
    maps = np.empty((N, H, W * wide, 3), np.uint8) if with_map else None
    vals = np.empty((N, H, W), np.float32) if with_float else None
    recs: List[DeltaE] = []

    def per_chunk(ctx, i, n, d_a, d_b, d_rec, d_map, d_val):
        if observer is not None:
            receptor_delta_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, observer=observer, mode=mode, gain=gain, threshold=threshold, layout=layout,
                                  d_float=d_val, acuity=acuity)
        elif ppd is None:
            delta_e_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, mode=mode, gain=gain, threshold=threshold, layout=layout, d_float=d_val)
        else:
            scielab_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, ppd=ppd, mode=mode, gain=gain, threshold=threshold, layout=layout, d_float=d_val)
        if with_map:
            ctx.download(d_map, (n, H, W * wide, 3), np.uint8, out=maps[i : i + n])
        recs.extend(delta_e_records_from_bytes(ctx.download(d_rec, (n * DELTA_E_RECORD_BYTES,), np.uint8), n))
        if with_float:
            ctx.download(d_val, (n, H, W), np.float32, out=vals[i : i + n])

    _walk(ctx, a, b, per_chunk, (DELTA_E_RECORD_BYTES, H * W * 3 * wide if with_map else None, H * W * 4 if with_float else None))
    return maps, recs, vals


def delta_e(a, b, *, threshold=DELTA_E_DEFAULT_THRESHOLD, ctx: Optional[Context] = None):
    """a, b: uint8 sRGB H x W x 3 -> the DeltaE record, or N x H x W x 3 -> a list of N; no map is computed.  Uploaded in chunks of at
    most 16 frames.  ValueError for a bad option or shape before any device work."""
    a, b, batched = check_pair(a, b)
    check_delta_e_options("heat", None, threshold, "map")
    recs = _delta_e_chunks(a, b, "heat", None, threshold, "map", ctx, False, False)[1]
    return recs if batched else recs[0]


def delta_e_map(a, b, *, mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD, layout: str = "map", ctx: Optional[Context] = None):
    """a, b: uint8 sRGB H x W x 3 -> (the map, uint8 H x W x 3 -- H x 3W x 3 with layout "side" --, its DeltaE record), or
    N x H x W x 3 -> (N maps, a list of N records).  mode: "heat" or "plain"; gain: 10 when None."""
    a, b, batched = check_pair(a, b)
    check_delta_e_options(mode, gain, threshold, layout)
    maps, recs, _ = _delta_e_chunks(a, b, mode, gain, threshold, layout, ctx, True, False)
    return (maps, recs) if batched else (maps[0], recs[0])


def delta_e_values(a, b, *, ctx: Optional[Context] = None) -> np.ndarray:
    """a, b: uint8 sRGB H x W x 3 -> the CIEDE2000 difference of every pixel, float32 H x W; N x H x W x 3 -> N x H x W."""
    a, b, batched = check_pair(a, b)
    vals = _delta_e_chunks(a, b, "heat", None, DELTA_E_DEFAULT_THRESHOLD, "map", ctx, False, True)[2]
    return vals if batched else vals[0]


# ------------------------------------------------------------------------------------------------ S-CIELAB
SCIELAB_MIN_PPD, SCIELAB_MAX_PPD = 2.0, 128.0


def check_ppd(ppd) -> float:
    """ppd -- pixels per degree of visual angle: pixels per unit length x viewing distance x tan 1 degree -- as the number the library
    takes, after avx_scielab_u8's check: a finite number from 2 to 128.  ValueError naming it otherwise."""
    if isinstance(ppd, bool) or not isinstance(ppd, numbers.Real) or not (math.isfinite(ppd) and SCIELAB_MIN_PPD <= ppd <= SCIELAB_MAX_PPD):
        raise ValueError(f"ppd must be a finite number from {SCIELAB_MIN_PPD:g} to {SCIELAB_MAX_PPD:g} (got {ppd!r})")
    return float(ppd)


def scielab_launch(ctx: Context, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, d_map: Optional[DeviceBuffer],
                   d_rec: DeviceBuffer, *, ppd, mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD, layout: str = "map",
                   d_float: Optional[DeviceBuffer] = None, stream=None) -> None:
    """delta_e_launch with both frames filtered for a viewer at `ppd` pixels per degree first (S-CIELAB): the same buffers, records
    and map.  Nothing is downloaded and nothing waits."""
    _check_call(n_frames, H, W, d_a, d_b)
    ppd = check_ppd(ppd)
    g, t = _check_delta_e_buffers(n_frames, H, W, d_map, d_rec, d_float, mode, gain, threshold, layout)
    ctx._check(lib.avx_scielab_u8(ctx._h, d_a.ptr, d_b.ptr, int(n_frames), int(H), int(W), ppd, AVX_DELTA_E_MODES[mode], g, t,
                                  AVX_DELTA_E_LAYOUTS[layout], None if d_map is None else d_map.ptr, d_rec.ptr,
                                  None if d_float is None else d_float.ptr, ctx._s(stream)))


def scielab(a, b, *, ppd, threshold=DELTA_E_DEFAULT_THRESHOLD, ctx: Optional[Context] = None):
    """delta_e at `ppd` pixels per degree: a, b uint8 sRGB H x W x 3 -> the DeltaE record, or N x H x W x 3 -> a list of N.  ValueError
    for a bad option or shape before any device work."""
    a, b, batched = check_pair(a, b)
    ppd = check_ppd(ppd)
    check_delta_e_options("heat", None, threshold, "map")
    recs = _delta_e_chunks(a, b, "heat", None, threshold, "map", ctx, False, False, ppd)[1]
    return recs if batched else recs[0]


def scielab_map(a, b, *, ppd, mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD, layout: str = "map", ctx: Optional[Context] = None):
    """delta_e_map at `ppd` pixels per degree; the dim grey and the A and B panels are the unfiltered frames'."""
    a, b, batched = check_pair(a, b)
    ppd = check_ppd(ppd)
    check_delta_e_options(mode, gain, threshold, layout)
    maps, recs, _ = _delta_e_chunks(a, b, mode, gain, threshold, layout, ctx, True, False, ppd)
    return (maps, recs) if batched else (maps[0], recs[0])


def scielab_values(a, b, *, ppd, ctx: Optional[Context] = None) -> np.ndarray:
    """delta_e_values at `ppd` pixels per degree: the S-CIELAB dE00 of every pixel, float32 H x W or N x H x W."""
    a, b, batched = check_pair(a, b)
    ppd = check_ppd(ppd)
    vals = _delta_e_chunks(a, b, "heat", None, DELTA_E_DEFAULT_THRESHOLD, "map", ctx, False, True, ppd)[2]
    return vals if batched else vals[0]


# ------------------------------------------------------------------------------------------------ receptor-noise-limited distance
RECEPTOR_MIN_WEBER, RECEPTOR_MAX_WEBER = 0.01, 1.0
RECEPTOR_MIN_FLOOR, RECEPTOR_MAX_FLOOR = 1e-6, 0.1
RECEPTOR_DEFAULT_FLOOR = 1e-3


def _real(v) -> bool:
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


@dataclasses.dataclass(frozen=True)
class Observer:
    """Who looks (avx_receptor_desc, include/avx.h): K = 2, 3 or 4 receptor classes as the K x 3 `matrix` on linear RGB (entries finite
    and not negative, no zero row; the library divides every row by its sum, so white has catch 1 in every class), the Weber fraction
    of every class in `weber` (0.01 .. 1: the noise of the class, the caller's choice -- there is no per-species table) and the
    `floor` (1e-6 .. 0.1) added to every catch before the logarithm.  matrix and weber are kept as tuples of floats.  ValueError
    naming the field otherwise."""

    name: str
    matrix: Tuple[Tuple[float, float, float], ...]
    weber: Tuple[float, ...]
    floor: float = RECEPTOR_DEFAULT_FLOOR

    def __post_init__(self):
        try:
            m = np.array(self.matrix, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"matrix must be K x 3 numbers (got {self.matrix!r})") from None
        if m.ndim != 2 or m.shape[1] != 3 or not 2 <= m.shape[0] <= 4:
            raise ValueError(f"matrix must be K x 3 with K = 2, 3 or 4 receptor classes (got shape {m.shape})")
        if not np.isfinite(m).all() or (m < 0).any():
            raise ValueError(f"matrix entries must be finite and not negative (got {m.tolist()})")
        for i, row in enumerate(m):
            if not (row.sum() > 0 and math.isfinite(row.sum())):
                raise ValueError(f"matrix row {i} sums to {row.sum():g}: it must be above 0")
        w = self.weber
        if isinstance(w, (str, bytes)) or not hasattr(w, "__len__") or len(w) != m.shape[0]:
            raise ValueError(f"weber must hold one Weber fraction per receptor class, {m.shape[0]} (got {w!r})")
        for i, e in enumerate(w):
            if not _real(e) or not RECEPTOR_MIN_WEBER <= e <= RECEPTOR_MAX_WEBER:
                raise ValueError(f"weber[{i}] must be a number from {RECEPTOR_MIN_WEBER:g} to {RECEPTOR_MAX_WEBER:g} (got {e!r})")
        if not _real(self.floor) or not RECEPTOR_MIN_FLOOR <= self.floor <= RECEPTOR_MAX_FLOOR:
            raise ValueError(f"floor must be a number from {RECEPTOR_MIN_FLOOR:g} to {RECEPTOR_MAX_FLOOR:g} (got {self.floor!r})")
        object.__setattr__(self, "name", str(self.name))
        object.__setattr__(self, "matrix", tuple(tuple(float(v) for v in row) for row in m))
        object.__setattr__(self, "weber", tuple(float(e) for e in w))
        object.__setattr__(self, "floor", float(self.floor))

    @property
    def n_receptors(self) -> int:
        return len(self.matrix)

    def desc(self) -> ReceptorDesc:
        """The avx_receptor_desc of this observer."""
        d = ReceptorDesc()
        d.struct_size, d.n_receptors, d.floor = ctypes.sizeof(ReceptorDesc), self.n_receptors, self.floor
        for i, row in enumerate(self.matrix):
            d.matrix[3 * i : 3 * i + 3] = row
        d.weber[: self.n_receptors] = self.weber
        return d

    def describe(self) -> str:
        """"Dog, weber 0.05,0.05, floor 0.001"."""
        return f"{self.name}, weber {','.join(f'{e:g}' for e in self.weber)}, floor {self.floor:g}"


def observer_names() -> List[str]:
    """The display names observer_for takes: the 20 dichromats, then HoneyBee."""
    from .gallery import NON_UV_NAMES

    return list(NON_UV_NAMES) + ["HoneyBee"]


def observer_for(species, weber, floor=RECEPTOR_DEFAULT_FLOOR) -> Observer:
    """The Observer of a species -- a display name (observer_names()), a class or an instance -- with the caller's Weber fractions.
    A dichromat has K = 2 classes in the order (LM, S): alpha L + (1 - alpha) M with the species' alpha, and S, of dichromat.py's
    RGB -> LMS matrix (s_scale cancels in a ratio).  HoneyBee has K = 3 in the order (UV, Blue, Green): its operator's rgb_matrix
    (an instance's own, with its illuminant and curves).  ValueError naming anything else: the UV plane-program species, MantisShrimp
    and RatUV have no K x 3 matrix on RGB."""
    from . import animals
    from .animals._dichromats import _Dichromat
    from .dichromat import M_RGB_TO_LMS
    from .gallery import species_class

    if isinstance(species, str):
        if species not in observer_names():
            raise ValueError(f"no receptor model on RGB for {species!r}: the observers are {', '.join(observer_names())}")
        name, who = species, species_class(species)
    else:
        who = species
        name = (who if isinstance(who, type) else type(who)).__name__
    cls = who if isinstance(who, type) else type(who)
    if issubclass(cls, _Dichromat):
        lms = M_RGB_TO_LMS.astype(np.float64)
        alpha = float(cls.SPEC.alpha)
        matrix = np.stack([alpha * lms[0] + (1.0 - alpha) * lms[1], lms[2]])
    elif issubclass(cls, animals.HoneyBee):
        bee = who() if isinstance(who, type) else who
        matrix = np.asarray(bee._operator().rgb_matrix, np.float64)
    else:
        raise ValueError(f"no receptor model on RGB for {name!r}: the observers are {', '.join(observer_names())}")
    return Observer(name, matrix, tuple(weber) if hasattr(weber, "__iter__") and not isinstance(weber, (str, bytes)) else weber, floor)


def _check_observer(observer) -> Observer:
    if not isinstance(observer, Observer):
        raise ValueError(f"observer must be an Observer, as observer_for(species, weber) builds one (got {type(observer).__name__})")
    return observer


# ------------------------------------------------------------------------------------------------ the observer's acuity
ACUITY_MIN_SIGMA, ACUITY_MAX_SIGMA = 0.2, 4.0
ACUITY_MAX_KSIZE = 33  # AVX_MAX_KSIZE


def check_acuity(sigma) -> float:
    """sigma -- the observer's acuity as the standard deviation of a Gaussian, in pixels of the frames as compared -- as the number the
    library takes, after avx_receptor_acuity_u8's check: finite, from 0.2 to 4, which keeps the cvRound(8 sigma + 1) | 1 taps at or
    below 33.  ValueError naming it otherwise."""
    from .dichromat import cv_auto_ksize

    if not _real(sigma) or not (math.isfinite(sigma) and ACUITY_MIN_SIGMA <= sigma <= ACUITY_MAX_SIGMA):
        raise ValueError(f"acuity must be a finite number of pixels from {ACUITY_MIN_SIGMA:g} to {ACUITY_MAX_SIGMA:g} (got {sigma!r})")
    k = cv_auto_ksize(float(sigma))
    if not 3 <= k <= ACUITY_MAX_KSIZE:
        raise ValueError(f"acuity {sigma!r} needs {k} taps: 3 to {ACUITY_MAX_KSIZE} are supported")
    return float(sigma)


def acuity_taps(sigma) -> np.ndarray:
    """The taps avx_receptor_acuity_u8 forms for `sigma`: dichromat.gaussian_taps(dichromat.cv_auto_ksize(sigma), sigma) -- what the
    species' own rendering blurs with -- formed in float64 and rounded once to float32."""
    from .dichromat import cv_auto_ksize, gaussian_taps

    sigma = check_acuity(sigma)
    return gaussian_taps(cv_auto_ksize(sigma), sigma).astype(np.float32)


def species_acuity(name: str) -> float:
    """The sigma, in pixels, of the Gaussian a species' own rendering ends with (its DichromatSpec: post == "gauss"): Dog 3.5, Squirrel
    0.7, Elephant 1.8, Lion 1.2, Tiger 1.2, Bear 1.6, Wolf 1.4, Fox 1.3, Raccoon 2.0, Cat 1.0.  ValueError, by name and with the reason,
    for every other observer: for those the caller gives a number."""
    from .animals._dichromats import _Dichromat
    from .gallery import species_class

    if not isinstance(name, str) or name not in observer_names():
        raise ValueError(f"no receptor model on RGB for {name!r}: the observers are {', '.join(observer_names())}")
    cls = species_class(name)
    if not issubclass(cls, _Dichromat):
        raise ValueError(f"{name} has no acuity blur: its rendering ends without one; give the acuity as a number of pixels")
    spec = cls.SPEC
    if spec.post == "scone":
        raise ValueError(f"{name} has no acuity blur: its rendering ends with a gain per image row; give the acuity as a number of pixels")
    if spec.post == "streak":
        raise ValueError(f"{name} has no single acuity: the blur of its visual streak is anisotropic and differs per image row; give the acuity as a "
                         "number of pixels")
    if spec.post != "gauss":
        raise ValueError(f"{name} has no acuity blur (post stage {spec.post!r}); give the acuity as a number of pixels")
    return check_acuity(float(spec.sigma))


def receptor_delta_launch(ctx: Context, d_a: DeviceBuffer, d_b: DeviceBuffer, n_frames: int, H: int, W: int, d_map: Optional[DeviceBuffer],
                          d_rec: DeviceBuffer, *, observer: Observer, mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD,
                          layout: str = "map", d_float: Optional[DeviceBuffer] = None, stream=None, acuity=None) -> None:
    """delta_e_launch with the receptor-noise-limited distance dS of `observer` in place of dE00: the same buffers, records and map;
    the threshold is in just-noticeable differences.  acuity: None, the distance per pixel of the frames as given; a number (0.2 .. 4),
    the sigma in pixels of the Gaussian both frames are blurred with, in linear light, before the catches are taken
    (avx_receptor_acuity_u8).  Nothing is downloaded and nothing waits."""
    _check_call(n_frames, H, W, d_a, d_b)
    desc = _check_observer(observer).desc()
    g, t = _check_delta_e_buffers(n_frames, H, W, d_map, d_rec, d_float, mode, gain, threshold, layout)
    if acuity is not None:
        sigma = check_acuity(acuity)
        ctx._check(lib.avx_receptor_acuity_u8(ctx._h, d_a.ptr, d_b.ptr, int(n_frames), int(H), int(W), ctypes.byref(desc), sigma,
                                              AVX_DELTA_E_MODES[mode], g, t, AVX_DELTA_E_LAYOUTS[layout], None if d_map is None else d_map.ptr, d_rec.ptr,
                                              None if d_float is None else d_float.ptr, ctx._s(stream)))
        return
    ctx._check(lib.avx_receptor_delta_u8(ctx._h, d_a.ptr, d_b.ptr, int(n_frames), int(H), int(W), ctypes.byref(desc), AVX_DELTA_E_MODES[mode], g, t,
                                         AVX_DELTA_E_LAYOUTS[layout], None if d_map is None else d_map.ptr, d_rec.ptr,
                                         None if d_float is None else d_float.ptr, ctx._s(stream)))


def _check_acuity_option(acuity) -> Optional[float]:
    return None if acuity is None else check_acuity(acuity)


def receptor_delta(a, b, observer: Observer, threshold=DELTA_E_DEFAULT_THRESHOLD, *, acuity=None, ctx: Optional[Context] = None):
    """How far apart `observer` sees a and b: uint8 sRGB H x W x 3 -> the DeltaE record of dS (just-noticeable differences), or
    N x H x W x 3 -> a list of N; no map is computed.  The measure is chromatic: two greys are 0 apart whatever their brightness.
    acuity: None, or the sigma in pixels of the observer's acuity blur (receptor_delta_launch; species_acuity(name) for a species' own).
    ValueError for a bad option or shape before any device work."""
    a, b, batched = check_pair(a, b)
    _check_observer(observer)
    acuity = _check_acuity_option(acuity)
    check_delta_e_options("heat", None, threshold, "map")
    recs = _delta_e_chunks(a, b, "heat", None, threshold, "map", ctx, False, False, observer=observer, acuity=acuity)[1]
    return recs if batched else recs[0]


def receptor_delta_map(a, b, observer: Observer, *, mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD, layout: str = "map",
                       acuity=None, ctx: Optional[Context] = None):
    """delta_e_map of dS as `observer` sees it: (the map, its DeltaE record), or (N maps, a list of N records).  With an acuity the dim
    grey and the A and B panels are still the unfiltered frames'."""
    a, b, batched = check_pair(a, b)
    _check_observer(observer)
    acuity = _check_acuity_option(acuity)
    check_delta_e_options(mode, gain, threshold, layout)
    maps, recs, _ = _delta_e_chunks(a, b, mode, gain, threshold, layout, ctx, True, False, observer=observer, acuity=acuity)
    return (maps, recs) if batched else (maps[0], recs[0])


def receptor_delta_values(a, b, observer: Observer, *, acuity=None, ctx: Optional[Context] = None) -> np.ndarray:
    """delta_e_values of dS as `observer` sees it: float32 H x W or N x H x W."""
    a, b, batched = check_pair(a, b)
    _check_observer(observer)
    acuity = _check_acuity_option(acuity)
    vals = _delta_e_chunks(a, b, "heat", None, DELTA_E_DEFAULT_THRESHOLD, "map", ctx, False, True, observer=observer, acuity=acuity)[2]
    return vals if batched else vals[0]


# ------------------------------------------------------------------------------------------------ receptor contrast within a frame
EDGES_CHANNELS = tuple(AVX_EDGES_CHANNELS)
EDGES_MAX_STEP = 8


def check_achromatic(observer: Observer, achromatic) -> Optional[LuminanceDesc]:
    """achromatic -- None, or (classes, weber): the 1-based numbers of the observer's receptor classes that feed its luminance channel
    and that channel's Weber fraction (0.01 .. 1, the caller's: there is no per-species table) -- as the avx_luminance_desc the library
    takes: the row is the mean of those classes' normalised rows.  ValueError naming it otherwise."""
    if achromatic is None:
        return None
    try:
        classes, weber = achromatic
        classes = tuple(classes)
    except (TypeError, ValueError):
        raise ValueError(f"achromatic must be (classes, weber), e.g. ((1,), 0.1) (got {achromatic!r})") from None
    K = observer.n_receptors
    if not classes or len(set(classes)) != len(classes):
        raise ValueError(f"achromatic classes must name at least one receptor class, each once (got {classes!r})")
    for k in classes:
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= K:
            raise ValueError(f"achromatic class {k!r} is not one of {observer.name}'s receptor classes 1..{K}")
    if not _real(weber) or not RECEPTOR_MIN_WEBER <= weber <= RECEPTOR_MAX_WEBER:
        raise ValueError(f"achromatic weber must be a number from {RECEPTOR_MIN_WEBER:g} to {RECEPTOR_MAX_WEBER:g} (got {weber!r})")
    m = np.array(observer.matrix, np.float64)
    m = m / m.sum(axis=1, keepdims=True)
    d = LuminanceDesc()
    d.struct_size, d.weber = ctypes.sizeof(LuminanceDesc), float(weber)
    d.row[:] = [float(v) for v in m[[k - 1 for k in classes]].mean(axis=0)]
    return d


SMOOTH_MAX_RADIUS, SMOOTH_MAX_ITERATIONS = 5, 8


def check_smooth(smooth) -> Optional[SmoothDesc]:
    """smooth -- None, or (radius, keep[, iterations = 1]): the edge-preserving smoothing in receptor space in front of the edges
    (avx_receptor_edges_smooth_u8): the window reaches `radius` pixels (1..5) each way, a pixel is averaged with about the
    share `keep` (above 0, at most 1) of its window that looks most like it, `iterations` times (0..8; 0 takes the planes route and
    smooths nothing) -- as the avx_smooth_desc the library takes.  ValueError naming it otherwise."""
    if smooth is None:
        return None
    try:
        radius, keep, *rest = smooth
        (iterations,) = rest or (1,)
    except (TypeError, ValueError):
        raise ValueError(f"smooth must be (radius, keep) or (radius, keep, iterations), e.g. (3, 0.5, 2) (got {smooth!r})") from None
    if isinstance(radius, bool) or not isinstance(radius, numbers.Integral) or not 1 <= radius <= SMOOTH_MAX_RADIUS:
        raise ValueError(f"smooth radius must be a whole number of pixels from 1 to {SMOOTH_MAX_RADIUS} (got {radius!r})")
    if not _real(keep) or not (math.isfinite(keep) and 0.0 < keep <= 1.0):
        raise ValueError(f"smooth keep must be a number above 0 and at most 1 (got {keep!r})")
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral) or not 0 <= iterations <= SMOOTH_MAX_ITERATIONS:
        raise ValueError(f"smooth iterations must be a whole number from 0 to {SMOOTH_MAX_ITERATIONS} (got {iterations!r})")
    d = SmoothDesc()
    d.struct_size, d.radius, d.keep, d.iterations = ctypes.sizeof(SmoothDesc), int(radius), float(keep), int(iterations)
    return d


def check_edges_options(observer, achromatic=None, channel=None, acuity=None, step=1, smooth=None):
    """(the luminance desc or None, the channel's name, sigma -- 0.0 without an acuity --, step) after the checks of
    avx_receptor_edges_u8 that need no device.  channel: "chromatic", "achromatic" or "either"; None is "either" with an achromatic
    channel, else "chromatic".  acuity: None, a number (check_acuity) or "species" (species_acuity of the observer's name).  smooth: None
    or what check_smooth takes; it is checked and not returned.  ValueError naming the option otherwise."""
    observer = _check_observer(observer)
    lum = check_achromatic(observer, achromatic)
    if channel is None:
        channel = "chromatic" if lum is None else "either"
    if channel not in AVX_EDGES_CHANNELS:
        raise ValueError(f"channel must be one of {', '.join(AVX_EDGES_CHANNELS)} (got {channel!r})")
    if channel != "chromatic" and lum is None:
        raise ValueError(f"channel {channel!r} needs achromatic=(classes, weber): without it the observer has no luminance channel")
    if isinstance(acuity, str):
        if acuity != "species":
            raise ValueError(f"acuity must be None, a number of pixels or 'species' (got {acuity!r})")
        sigma = species_acuity(observer.name)
    else:
        sigma = 0.0 if acuity is None else check_acuity(acuity)
    if isinstance(step, bool) or not isinstance(step, numbers.Integral) or not 1 <= step <= EDGES_MAX_STEP:
        raise ValueError(f"step must be a whole number of pixels from 1 to {EDGES_MAX_STEP} (got {step!r})")
    check_smooth(smooth)
    return lum, channel, sigma, int(step)


def edges_planes(observer: Observer, channel: str) -> int:
    """P, the planes of log-catches a channel works on: the K receptor planes for "chromatic", the luminance plane for "achromatic",
    K + 1 for "either"."""
    return (0 if channel == "achromatic" else observer.n_receptors) + (0 if channel == "chromatic" else 1)


def receptor_edges_launch(ctx: Context, d_in: DeviceBuffer, n_frames: int, H: int, W: int, d_map: Optional[DeviceBuffer], d_rec: DeviceBuffer, *,
                          observer: Observer, achromatic=None, channel=None, acuity=None, step: int = 1, mode: str = "heat", gain=None,
                          threshold=DELTA_E_DEFAULT_THRESHOLD, d_float: Optional[DeviceBuffer] = None, stream=None, smooth=None,
                          d_planes: Optional[DeviceBuffer] = None) -> None:
    """Enqueue avx_receptor_edges_u8 on `stream`: per pixel of n_frames uint8 sRGB frames in d_in the largest receptor-noise-limited
    contrast, as `observer` sees it, between the pixel and its up to eight neighbours `step` pixels away -- chromatic, achromatic (the
    luminance channel that `achromatic` names) or either -- behind the acuity blur when there is one.  d_rec takes n_frames records of
    DELTA_E_RECORD_BYTES; d_map, when not None, n_frames maps of H x W x 3; d_float, when not None, the float32 values.  smooth: None,
    or (radius, keep[, iterations]) -- check_smooth -- for avx_receptor_edges_smooth_u8: the edge-preserving smoothing in receptor space
    in front of the edges; d_planes, which needs it, takes the smoothed planes, n_frames x P x H x W float32 (edges_planes(observer,
    channel) says P).  Nothing is downloaded and nothing waits."""
    _check_call(n_frames, H, W, d_in, d_in)
    lum, channel, sigma, step = check_edges_options(observer, achromatic, channel, acuity, step)
    sm = check_smooth(smooth)
    desc = observer.desc()
    g, t = _check_delta_e_buffers(n_frames, H, W, d_map, d_rec, d_float, mode, gain, threshold, "map")
    if sm is None and d_planes is not None:
        raise ValueError("d_planes takes the smoothed planes: it needs smooth=(radius, keep[, iterations])")
    if sm is not None:
        need = n_frames * edges_planes(observer, channel) * H * W * 4
        if d_planes is not None and d_planes.nbytes < need:
            raise ValueError(f"d_planes holds {d_planes.nbytes} bytes, the planes need {need}")
        ctx._check(lib.avx_receptor_edges_smooth_u8(ctx._h, d_in.ptr, int(n_frames), int(H), int(W), ctypes.byref(desc), None if lum is None else ctypes.byref(lum),
                                                    AVX_EDGES_CHANNELS[channel], sigma, step, ctypes.byref(sm), AVX_DELTA_E_MODES[mode], g, t,
                                                    None if d_map is None else d_map.ptr, d_rec.ptr, None if d_float is None else d_float.ptr,
                                                    None if d_planes is None else d_planes.ptr, ctx._s(stream)))
        return
    ctx._check(lib.avx_receptor_edges_u8(ctx._h, d_in.ptr, int(n_frames), int(H), int(W), ctypes.byref(desc), None if lum is None else ctypes.byref(lum),
                                         AVX_EDGES_CHANNELS[channel], sigma, step, AVX_DELTA_E_MODES[mode], g, t, None if d_map is None else d_map.ptr,
                                         d_rec.ptr, None if d_float is None else d_float.ptr, ctx._s(stream)))


def _check_frames(frames):
    """uint8 H x W x 3 or N x H x W x 3 -> the contiguous 4-D array and whether a frame axis was given."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        raise ValueError(f"frames are uint8 (got {frames.dtype} {frames.shape})")
    if frames.ndim not in (3, 4) or frames.shape[-1] != 3 or 0 in frames.shape:
        raise ValueError(f"expected H x W x 3 or N x H x W x 3 (got {frames.shape})")
    batched = frames.ndim == 4
    return np.ascontiguousarray(frames if batched else frames[None]), batched


def _edges_chunks(frames, observer, opts, mode, gain, threshold, ctx, with_map, with_float, with_planes=False):
    """receptor_edges, receptor_edges_map, receptor_edges_values and receptor_smooth_planes: the stack in chunks of at most 16 frames ->
    (maps or None, records, values or None, planes or None)."""
    N, H, W = frames.shape[:3]
    ctx = ctx or get_context()
    chunk = min(N, MAX_FRAMES)
    maps = np.empty((N, H, W, 3), np.uint8) if with_map else None
    vals = np.empty((N, H, W), np.float32) if with_float else None
    P = edges_planes(observer, check_edges_options(observer, opts["achromatic"], opts["channel"])[1]) if with_planes else 0
    planes = np.empty((N, P, H, W), np.float32) if with_planes else None
    recs: List[DeltaE] = []
    bufs = []
    try:
        d_in, d_rec = ctx.malloc(chunk * H * W * 3), ctx.malloc(chunk * DELTA_E_RECORD_BYTES)
        bufs += [d_in, d_rec]
        d_map = ctx.malloc(chunk * H * W * 3) if with_map else None
        d_val = ctx.malloc(chunk * H * W * 4) if with_float else None
        d_pl = ctx.malloc(chunk * P * H * W * 4) if with_planes else None
        bufs += [d for d in (d_map, d_val, d_pl) if d is not None]
        for i in range(0, N, chunk):
            n = min(chunk, N - i)
            ctx.upload(frames[i : i + n], d_in)
            receptor_edges_launch(ctx, d_in, n, H, W, d_map, d_rec, observer=observer, mode=mode, gain=gain, threshold=threshold, d_float=d_val,
                                  d_planes=d_pl, **opts)
            if with_map:
                ctx.download(d_map, (n, H, W, 3), np.uint8, out=maps[i : i + n])
            recs.extend(delta_e_records_from_bytes(ctx.download(d_rec, (n * DELTA_E_RECORD_BYTES,), np.uint8), n))
            if with_float:
                ctx.download(d_val, (n, H, W), np.float32, out=vals[i : i + n])
            if with_planes:
                ctx.download(d_pl, (n, P, H, W), np.float32, out=planes[i : i + n])
    finally:
        for d in bufs:
            d.free()
    return maps, recs, vals, planes


def _edges_call(frames, observer, achromatic, channel, acuity, step, mode, gain, threshold, smooth=None):
    """The checks that the three array entries make before any device work."""
    frames, batched = _check_frames(frames)
    check_edges_options(observer, achromatic, channel, acuity, step, smooth)
    check_delta_e_options(mode, gain, threshold, "map")
    return frames, batched, dict(achromatic=achromatic, channel=channel, acuity=acuity, step=step, smooth=smooth)


def receptor_edges(frames, observer: Observer, *, achromatic=None, channel=None, acuity=None, step: int = 1, threshold=DELTA_E_DEFAULT_THRESHOLD,
                   smooth=None, ctx: Optional[Context] = None):
    """What stands out to `observer` within a frame: uint8 sRGB H x W x 3 -> the DeltaE record of the per-pixel edge value (the largest
    contrast to a neighbour `step` pixels away, in just-noticeable differences), or N x H x W x 3 -> a list of N; no map is computed.
    achromatic=(classes, weber) gives the observer a luminance channel (check_achromatic); channel picks "chromatic", "achromatic" or
    "either" (the default with a luminance channel; without one, "chromatic"); acuity is None, a sigma in pixels or "species".
    smooth=(radius, keep[, iterations]) puts the edge-preserving smoothing of DESIGN §4.29 in front of the edges (check_smooth): the
    project's stand-in for QCPA's RNL ranked filter; it smooths in the channel of the edges, so "either" is then no longer the larger of
    the two single-channel results.  ValueError for a bad option or shape before any device work."""
    frames, batched, opts = _edges_call(frames, observer, achromatic, channel, acuity, step, "heat", None, threshold, smooth)
    recs = _edges_chunks(frames, observer, opts, "heat", None, threshold, ctx, False, False)[1]
    return recs if batched else recs[0]


def receptor_edges_map(frames, observer: Observer, *, achromatic=None, channel=None, acuity=None, step: int = 1, mode: str = "heat", gain=None,
                       threshold=DELTA_E_DEFAULT_THRESHOLD, smooth=None, ctx: Optional[Context] = None):
    """receptor_edges with the picture: (the map, uint8 H x W x 3, its DeltaE record), or (N maps, a list of N records).  mode "heat":
    the dim grey of the frame where the value is within the threshold, the palette colour of gain x (value - threshold) elsewhere;
    "plain": the colour of gain x value everywhere.  With smooth the dim grey is still the unfiltered frame's."""
    frames, batched, opts = _edges_call(frames, observer, achromatic, channel, acuity, step, mode, gain, threshold, smooth)
    maps, recs = _edges_chunks(frames, observer, opts, mode, gain, threshold, ctx, True, False)[:2]
    return (maps, recs) if batched else (maps[0], recs[0])


def receptor_edges_values(frames, observer: Observer, *, achromatic=None, channel=None, acuity=None, step: int = 1, smooth=None,
                          ctx: Optional[Context] = None) -> np.ndarray:
    """The edge value of every pixel: float32 H x W or N x H x W."""
    frames, batched, opts = _edges_call(frames, observer, achromatic, channel, acuity, step, "heat", None, DELTA_E_DEFAULT_THRESHOLD, smooth)
    vals = _edges_chunks(frames, observer, opts, "heat", None, DELTA_E_DEFAULT_THRESHOLD, ctx, False, True)[2]
    return vals if batched else vals[0]


def receptor_smooth_planes(frames, observer: Observer, *, achromatic=None, channel=None, acuity=None, smooth, ctx: Optional[Context] = None) -> np.ndarray:
    """The planes of log-catches the edges are taken on, after the smoothing (iterations 0: before it): float32 P x H x W, or
    N x P x H x W -- the K receptor planes for "chromatic", the luminance plane for "achromatic", the K and then the luminance plane for
    "either".  smooth is required: (radius, keep[, iterations])."""
    if smooth is None:
        raise ValueError("smooth must be (radius, keep) or (radius, keep, iterations): receptor_smooth_planes returns the smoothed planes")
    frames, batched, opts = _edges_call(frames, observer, achromatic, channel, acuity, 1, "heat", None, DELTA_E_DEFAULT_THRESHOLD, smooth)
    planes = _edges_chunks(frames, observer, opts, "heat", None, DELTA_E_DEFAULT_THRESHOLD, ctx, False, False, with_planes=True)[3]
    return planes if batched else planes[0]


# ------------------------------------------------------------------------------------------------ dE_ITP
ITP_DEFAULT_SDR_WHITE = 203.0


def check_sdr_white(sdr_white) -> float:
    """The nits of SDR code 255 as the number the library takes: finite and positive, ValueError otherwise."""
    if isinstance(sdr_white, bool) or not isinstance(sdr_white, numbers.Real) or not (math.isfinite(sdr_white) and sdr_white > 0.0):
        raise ValueError(f"sdr_white must be finite and positive (got {sdr_white!r})")
    return float(sdr_white)


class HdrFrames:
    """An HDR side of itp_delta: `payload` holds frames of H x W in one of the four 10-bit formats as they are stored (uint8, 16-bit
    samples as little-endian byte pairs, or uint16) -- one frame in any shape, or (N, frame bytes) --, BT.2020 Y'CbCr in `range`
    ("limited" or "full") with `transfer` "pq" or "hlg".  ValueError for a setting the HDR decode refuses or a payload of another size."""

    def __init__(self, payload, pix_fmt: str, H: int, W: int, transfer: str, range: str = "limited"):  # noqa: A002  (the decode's name for it)
        from .yuv import frame_size, hdr_codes

        hdr_codes(pix_fmt, transfer, range)
        a = np.ascontiguousarray(payload)
        if a.dtype == np.dtype("<u2"):
            a = a.view(np.uint8) if a.ndim else a.reshape(1).view(np.uint8)
        if a.dtype != np.uint8:
            raise ValueError(f"HDR payloads are uint8 or little-endian uint16 (got {a.dtype})")
        fsz = frame_size(pix_fmt, H, W)
        self.batched = a.ndim == 2 and a.shape[1] == fsz
        if not self.batched and a.size != fsz:
            raise ValueError(f"expected {fsz} bytes per {H}x{W} {pix_fmt} frame (or an (N, {fsz}) batch), got shape {a.shape}")
        self.payload = a if self.batched else a.reshape(1, fsz)
        self.pix_fmt, self.H, self.W, self.transfer, self.range = pix_fmt, int(H), int(W), transfer, range

    def __len__(self) -> int:
        return len(self.payload)

    def decode(self, tonemap: str = "mobius", peak_nits: float = 1000.0, sdr_white: float = ITP_DEFAULT_SDR_WHITE):
        """The yuv.Decode that makes this side's panel frames."""
        from .yuv import Decode

        return Decode(self.pix_fmt, range=self.range, transfer=self.transfer, tonemap=tonemap, peak_nits=peak_nits, sdr_white=sdr_white)


@dataclasses.dataclass
class ItpSide:
    """One side of itp_delta_launch on the device.  d_data: the frames -- uint8 sRGB H x W x 3 when pix_fmt is None, else the HDR
    payloads as stored (pix_fmt, transfer, range as HdrFrames takes them); d_panel: for an HDR side whose launch writes a map, its
    tone-mapped decode to uint8 RGB."""
    d_data: DeviceBuffer
    pix_fmt: Optional[str] = None
    transfer: Optional[str] = None
    range: str = "limited"
    d_panel: Optional[DeviceBuffer] = None

    @property
    def hdr(self) -> bool:
        return self.pix_fmt is not None

    def _struct(self, n_frames: int, H: int, W: int, with_map: bool) -> ItpSideStruct:
        from .yuv import frame_size, hdr_codes

        s = ItpSideStruct(struct_size=ctypes.sizeof(ItpSideStruct), kind=1 if self.hdr else 0, data=self.d_data.ptr)
        need = n_frames * (frame_size(self.pix_fmt, H, W) if self.hdr else H * W * 3)
        if self.d_data.nbytes < need:
            raise ValueError(f"{n_frames} frames of {H} x {W} need {need} bytes; the buffer holds {self.d_data.nbytes}")
        if self.hdr:
            s.pix_fmt, s.full_range, s.transfer = hdr_codes(self.pix_fmt, self.transfer, self.range)[:3]
            if with_map:
                if self.d_panel is None or self.d_panel.nbytes < n_frames * H * W * 3:
                    raise ValueError(f"a map needs the {n_frames} decoded panel frames of an HDR side ({n_frames * H * W * 3} bytes)")
                s.panel = self.d_panel.ptr
        return s


def itp_delta_launch(ctx: Context, a: ItpSide, b: ItpSide, n_frames: int, H: int, W: int, d_map: Optional[DeviceBuffer], d_rec: DeviceBuffer, *,
                     sdr_white=ITP_DEFAULT_SDR_WHITE, mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD, layout: str = "map",
                     d_float: Optional[DeviceBuffer] = None, stream=None) -> None:
    """delta_e_launch with dE_ITP in place of dE00 and sides of either kind: the same records, map and value plane.  sdr_white is the
    nits of code 255 of an SDR side.  Nothing is downloaded and nothing waits."""
    if not 1 <= n_frames <= MAX_FRAMES:
        raise ValueError(f"n_frames must be 1..{MAX_FRAMES} (got {n_frames})")
    if H < 1 or W < 1 or H * W >= 1 << 32:
        raise ValueError(f"bad frame size {H} x {W}")
    white = check_sdr_white(sdr_white)
    g, t = _check_delta_e_buffers(n_frames, H, W, d_map, d_rec, d_float, mode, gain, threshold, layout)
    sa, sb = a._struct(n_frames, H, W, d_map is not None), b._struct(n_frames, H, W, d_map is not None)
    ctx._check(lib.avx_itp_delta(ctx._h, ctypes.byref(sa), ctypes.byref(sb), white, int(n_frames), int(H), int(W), AVX_DELTA_E_MODES[mode], g, t,
                                 AVX_DELTA_E_LAYOUTS[layout], None if d_map is None else d_map.ptr, d_rec.ptr,
                                 None if d_float is None else d_float.ptr, ctx._s(stream)))


def _itp_sides(a, b):
    """The two sides as (array of N rows, HdrFrames or None) each, N, H, W and whether a frame axis was given."""
    out, shapes, batched = [], [], []
    for name, x in (("a", a), ("b", b)):
        if isinstance(x, HdrFrames):
            out.append((x.payload, x))
            shapes.append((len(x), x.H, x.W))
            batched.append(x.batched)
        else:
            x = np.asarray(x)
            if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] != 3 or 0 in x.shape:
                raise ValueError(f"{name}: an SDR side is uint8 H x W x 3 or N x H x W x 3; an HDR side is an HdrFrames (got {x.dtype} {x.shape})")
            batched.append(x.ndim == 4)
            x = np.ascontiguousarray(x if x.ndim == 4 else x[None])
            out.append((x, None))
            shapes.append(x.shape[:3])
    if shapes[0] != shapes[1]:
        raise ValueError(f"a and b differ in frames or size (a: {shapes[0][0]} of {shapes[0][1]} x {shapes[0][2]}, b: {shapes[1][0]} of {shapes[1][1]} x {shapes[1][2]})")
    return out, shapes[0], batched[0] or batched[1]


def _itp_chunks(a, b, sdr_white, mode, gain, threshold, layout, ctx, with_map, with_float, tonemap="mobius", peak_nits=1000.0):
    """itp_delta, itp_delta_map and itp_delta_values: the sides in chunks of at most 16 frames -> (maps or None, records, values or
    None, whether a frame axis was given)."""
    white = check_sdr_white(sdr_white)
    check_delta_e_options(mode, gain, threshold, layout)
    sides, (N, H, W), batched = _itp_sides(a, b)
    (xa, ha), (xb, hb) = sides
    wide = 3 if layout == "side" else 1
    maps = np.empty((N, H, W * wide, 3), np.uint8) if with_map else None
    vals = np.empty((N, H, W), np.float32) if with_float else None
    recs: List[DeltaE] = []
    decodes = [h.decode(tonemap, peak_nits, white) if (h is not None and with_map) else None for _, h in sides]

    def per_chunk(ctx, i, n, d_a, d_b, d_rec, d_map, d_val, d_pa, d_pb):
        launch_sides = []
        for d, h, dec, d_p in ((d_a, ha, decodes[0], d_pa), (d_b, hb, decodes[1], d_pb)):
            if dec is not None:
                dec.launch(ctx, d, d_p, n, H, W)
            launch_sides.append(ItpSide(d) if h is None else ItpSide(d, h.pix_fmt, h.transfer, h.range, d_p))
        itp_delta_launch(ctx, launch_sides[0], launch_sides[1], n, H, W, d_map, d_rec, sdr_white=white, mode=mode, gain=gain, threshold=threshold,
                         layout=layout, d_float=d_val)
        if with_map:
            ctx.download(d_map, (n, H, W * wide, 3), np.uint8, out=maps[i : i + n])
        recs.extend(delta_e_records_from_bytes(ctx.download(d_rec, (n * DELTA_E_RECORD_BYTES,), np.uint8), n))
        if with_float:
            ctx.download(d_val, (n, H, W), np.float32, out=vals[i : i + n])

    _walk(ctx, xa, xb, per_chunk, (DELTA_E_RECORD_BYTES, H * W * 3 * wide if with_map else None, H * W * 4 if with_float else None,
                                   H * W * 3 if decodes[0] is not None else None, H * W * 3 if decodes[1] is not None else None))
    return maps, recs, vals, batched


def itp_delta(a, b, sdr_white=ITP_DEFAULT_SDR_WHITE, *, threshold=DELTA_E_DEFAULT_THRESHOLD, ctx: Optional[Context] = None):
    """dE_ITP (BT.2124) of a against b.  A side is an HdrFrames or uint8 sRGB frames (H x W x 3 or N x H x W x 3) shown with code 255
    at sdr_white nits; any mix.  -> the DeltaE record, or a list of N when either side has a frame axis; no map is computed."""
    recs, batched = _itp_chunks(a, b, sdr_white, "heat", None, threshold, "map", ctx, False, False)[1::2]
    return recs if batched else recs[0]


def itp_delta_map(a, b, *, mode: str = "heat", gain=None, threshold=DELTA_E_DEFAULT_THRESHOLD, layout: str = "map", sdr_white=ITP_DEFAULT_SDR_WHITE,
                  tonemap: str = "mobius", peak_nits: float = 1000.0, ctx: Optional[Context] = None):
    """delta_e_map of dE_ITP: (the map, its DeltaE record), or (N maps, a list of N records).  The dim grey and the A and B panels of
    an HDR side are its decode with `tonemap`, `peak_nits` and `sdr_white`; an SDR side is shown as it is."""
    maps, recs, _, batched = _itp_chunks(a, b, sdr_white, mode, gain, threshold, layout, ctx, True, False, tonemap, peak_nits)
    return (maps, recs) if batched else (maps[0], recs[0])


def itp_delta_values(a, b, sdr_white=ITP_DEFAULT_SDR_WHITE, *, ctx: Optional[Context] = None) -> np.ndarray:
    """delta_e_values of dE_ITP: float32 H x W, or N x H x W when either side has a frame axis."""
    vals, batched = _itp_chunks(a, b, sdr_white, "heat", None, DELTA_E_DEFAULT_THRESHOLD, "map", ctx, False, True)[2:]
    return vals if batched else vals[0]
