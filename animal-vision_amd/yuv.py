"""YUV <-> RGB uint8 on the device, in the style of geometry.py: the I420 pair of the Y4M path (csrc/yuv.hip) and the raw video
pixel formats -- nv12, p010le, 4:2:2, 4:4:4, gray, 10-bit planar -- of csrc/yuv_raw.hip (PIX_FMTS), and the HDR decode
of csrc/yuv_hdr.hip: 10-bit BT.2020 PQ / HLG payloads -> tone-mapped SDR RGB (yuv_hdr_to_rgb); and the scaled decode
of csrc/yuv_scale.hip: a raw payload -> RGB at a smaller size in one launch, byte-equal to the decode followed by cv2's INTER_AREA
resize (yuv_to_rgb_scaled); and the scaled HDR decode of csrc/yuv_hdr_scale.hip: the two together, an HDR payload
-> tone-mapped SDR RGB at a smaller size in one launch (yuv_hdr_to_rgb_scaled).

The arithmetic (int32 fixed point, 16 fractional bits, BT.601 / BT.709, limited / full range) is defined in DESIGN §4.8; the
coefficient tables are built by the C entry points from the (matrix, range) names below.  A payload is one frame's Y plane
(H x W), then U and V (ceil(H/2) x ceil(W/2) each), frames back to back."""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import numpy as np

from ._lib import AVX_PIX_FMTS, AVX_TONEMAPS, AVX_TRANSFERS, lib
from .runtime import Context, DeviceBuffer, get_context

MATRICES = {"bt601": 0, "bt709": 1}  # AVX_YUV_BT601, AVX_YUV_BT709
RANGES = {"limited": 0, "full": 1}   # the full_range argument
PIX_FMTS = tuple(AVX_PIX_FMTS)       # ffmpeg's -pix_fmt names of the raw formats (include/avx.h: enum avx_pix_fmt)
TRANSFERS = ("pq", "hlg")            # HDR transfer functions of the HDR decode (enum avx_transfer)
TONEMAPS = ("clip", "mobius")        # enum avx_tonemap
HDR_PIX_FMTS = tuple(f for f in AVX_PIX_FMTS if f.endswith("10le"))  # the 10-bit formats: what the HDR decode reads


def i420_size(H: int, W: int) -> int:
    """Bytes of one I420 frame of H x W pixels."""
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def _codes(matrix: str, range: str):
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)} (got {matrix!r})")
    if range not in RANGES:
        raise ValueError(f"range must be one of {sorted(RANGES)} (got {range!r})")
    return MATRICES[matrix], RANGES[range]


def coefficients(matrix: str = "bt601", range: str = "limited", depth: int = 8):
    """The fixed-point tables the kernels run with, as the C side builds them: (cy, crv, cgu, cgv, cbu, yo) for the decode and
    ((Y row), (U row), (V row)), yo for the encode, each row an (r, g, b) triple of 16.16 coefficients.  depth: bits per
    sample, 8 or 10."""
    import ctypes

    m, r = _codes(matrix, range)
    dec, enc = (ctypes.c_int * 6)(), (ctypes.c_int * 10)()
    if lib.avx_yuv_coefficients_d(m, r, int(depth), dec, enc) != 0:
        raise ValueError(f"avx_yuv_coefficients_d({matrix!r}, {range!r}, depth={depth!r}) failed")
    e = list(enc)
    return tuple(dec), ((tuple(e[0:3]), tuple(e[3:6]), tuple(e[6:9])), e[9])


def _fmt_code(pix_fmt: str) -> int:
    if pix_fmt not in AVX_PIX_FMTS:
        raise ValueError(f"pix_fmt must be one of {', '.join(PIX_FMTS)} (got {pix_fmt!r})")
    return AVX_PIX_FMTS[pix_fmt]


def frame_size(pix_fmt: str, H: int, W: int) -> int:
    """Bytes of one H x W frame in `pix_fmt`."""
    n = int(lib.avx_yuv_frame_size(_fmt_code(pix_fmt), int(H), int(W)))
    if n == 0:
        raise ValueError(f"bad frame size {H} x {W}")
    return n


def hdr_codes(pix_fmt: str, transfer: str, range: str = "limited", tonemap: str = "mobius", peak_nits: float = 1000.0, sdr_white: float = 203.0):
    """Checks the settings of the HDR decode without touching the device; returns the C side's (fmt, full_range,
    transfer, tonemap, peak_nits, sdr_white)."""
    import math

    if pix_fmt not in HDR_PIX_FMTS:
        raise ValueError(f"the HDR decode reads the 10-bit formats {', '.join(HDR_PIX_FMTS)} (got pix_fmt={pix_fmt!r})")
    if transfer not in TRANSFERS:
        raise ValueError(f"transfer must be one of {', '.join(TRANSFERS)} (got {transfer!r})")
    if tonemap not in TONEMAPS:
        raise ValueError(f"tonemap must be one of {', '.join(TONEMAPS)} (got {tonemap!r})")
    if range not in RANGES:
        raise ValueError(f"range must be one of {sorted(RANGES)} (got {range!r})")
    try:
        peak, white = float(peak_nits), float(sdr_white)
    except (TypeError, ValueError):
        raise ValueError(f"peak_nits and sdr_white are numbers (got {peak_nits!r}, {sdr_white!r})")
    if not (math.isfinite(peak) and math.isfinite(white) and white > 0.0 and peak > white):
        raise ValueError(f"peak_nits and sdr_white must be finite and positive, with peak_nits > sdr_white (got {peak_nits!r}, {sdr_white!r})")
    return AVX_PIX_FMTS[pix_fmt], RANGES[range], AVX_TRANSFERS[transfer], AVX_TONEMAPS[tonemap], peak, white


def check_scale(H: int, W: int, Hd: int, Wd: int) -> None:
    """The sizes of a scaled decode: an H x W source reduced to Hd x Wd.  Enlarging on either axis (cv2 would switch
    to INTER_LINEAR there) and non-positive sizes are a ValueError that names both sizes."""
    try:
        ok = all(int(v) == v for v in (H, W, Hd, Wd))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"sizes are integers (got {W!r}x{H!r} -> {Wd!r}x{Hd!r})")
    if H < 1 or W < 1 or Hd < 1 or Wd < 1:
        raise ValueError(f"sizes must be positive (got {W}x{H} -> {Wd}x{Hd})")
    if Hd > H or Wd > W:
        raise ValueError(f"scale {Wd}x{Hd} enlarges the {W}x{H} source: the scaled decode only reduces (INTER_AREA)")


def _check_sizes(n_frames: int, H: int, W: int, d_rgb: DeviceBuffer, d_yuv: DeviceBuffer, pix_fmt: Optional[str] = None,
                 out_hw: Optional[Tuple[int, int]] = None) -> None:
    """The kernels read and write n_frames whole frames: an undersized buffer is an error here, before the launch.  The one size
    check of every entry point below: pix_fmt None is I420; out_hw is the (Hd, Wd) of the RGB frames of a scaled decode."""
    if n_frames < 1 or H < 1 or W < 1:
        raise ValueError(f"bad shape: {n_frames} frames of {H} x {W}")
    Hd, Wd = out_hw or (H, W)
    need_rgb, need_yuv = n_frames * Hd * Wd * 3, n_frames * (i420_size(H, W) if pix_fmt is None else frame_size(pix_fmt, H, W))
    if d_rgb.nbytes < need_rgb or d_yuv.nbytes < need_yuv:
        to = f" -> {Hd} x {Wd}" if out_hw else ""
        raise ValueError(f"{n_frames} frames of {H} x {W}{to} need {need_rgb} RGB and {need_yuv} {pix_fmt or 'I420'} bytes; "
                         f"the buffers hold {d_rgb.nbytes} and {d_yuv.nbytes}")


def _through_device(ctx: Optional[Context], a: np.ndarray, out_shape: tuple, launch) -> np.ndarray:
    """`a` uploaded, launch(ctx, d_in, d_out), the uint8 result of `out_shape` downloaded; both buffers are freed however it ends."""
    ctx = ctx or get_context()
    d_in = ctx.upload(a)
    d_out = ctx.malloc(int(np.prod(out_shape)))
    try:
        launch(ctx, d_in, d_out)
        return ctx.download(d_out, out_shape, np.uint8)
    finally:
        d_in.free()
        d_out.free()


# ---------------------------------------------------------------- a decode and an encode as values ---------------------------------
@dataclasses.dataclass(frozen=True)
class Decode:
    """How YUV payloads become RGB uint8 frames: settings only, the frame size is given at the call.  pix_fmt None is the I420 payload
    of a .y4m, else one of PIX_FMTS; with a `transfer` the payloads are HDR (a 10-bit pix_fmt; `tonemap`, `peak_nits` and `sdr_white`
    take the place of `matrix`); scale = (Wd, Hd) decodes straight to that smaller size.
    Construction checks everything that needs neither a size nor a device; launch is the one place that picks the C entry point."""
    pix_fmt: Optional[str] = None
    matrix: str = "bt601"
    range: str = "limited"
    transfer: Optional[str] = None
    tonemap: str = "mobius"
    peak_nits: float = 1000.0
    sdr_white: float = 203.0
    scale: Optional[Tuple[int, int]] = None

    def __post_init__(self):
        _codes(self.matrix, self.range)
        if self.pix_fmt is not None:
            _fmt_code(self.pix_fmt)
        if self.transfer is not None:
            hdr_codes(self.pix_fmt, self.transfer, self.range, self.tonemap, self.peak_nits, self.sdr_white)
        if self.scale is not None:
            try:
                Wd, Hd = self.scale
            except (TypeError, ValueError):
                raise ValueError(f"scale is (Wd, Hd) (got {self.scale!r})")
            object.__setattr__(self, "scale", (Wd, Hd))  # a tuple whatever sequence came: equal settings are equal values

    def frame_bytes(self, H: int, W: int) -> int:
        """Bytes of one H x W payload."""
        return i420_size(H, W) if self.pix_fmt is None else frame_size(self.pix_fmt, H, W)

    def out_hw(self, H: int, W: int) -> Tuple[int, int]:
        """(H, W) of the RGB frames an H x W source decodes to: the scale, checked against the source (check_scale), else the source's."""
        if self.scale is None:
            return H, W
        check_scale(H, W, self.scale[1], self.scale[0])
        return int(self.scale[1]), int(self.scale[0])

    def launch(self, ctx: Context, d_yuv: DeviceBuffer, d_rgb: DeviceBuffer, n_frames: int, H: int, W: int, stream=None) -> None:
        """n_frames payloads of H x W in d_yuv -> n_frames RGB frames of out_hw(H, W) in d_rgb: every check, then one launch."""
        Hd, Wd = self.out_hw(H, W)
        _check_sizes(n_frames, H, W, d_rgb, d_yuv, self.pix_fmt, (Hd, Wd) if self.scale is not None else None)
        fmt = AVX_PIX_FMTS[self.pix_fmt or "yuv420p"]  # yuv420p is the I420 payload, byte for byte (include/avx.h)
        m, r, n, H, W, s = MATRICES[self.matrix], RANGES[self.range], int(n_frames), int(H), int(W), ctx._s(stream)
        if self.transfer is not None:
            hdr = (r, AVX_TRANSFERS[self.transfer], AVX_TONEMAPS[self.tonemap], float(self.peak_nits), float(self.sdr_white), s)
            if self.scale is not None:
                rc = lib.avx_yuv_hdr_to_rgb_scaled_u8(ctx._h, fmt, d_yuv.ptr, d_rgb.ptr, n, H, W, Hd, Wd, *hdr)
            else:
                rc = lib.avx_yuv_hdr_to_rgb_u8(ctx._h, fmt, d_yuv.ptr, d_rgb.ptr, n, H, W, *hdr)
        elif self.scale is not None:
            rc = lib.avx_yuv_to_rgb_scaled_u8(ctx._h, fmt, d_yuv.ptr, d_rgb.ptr, n, H, W, Hd, Wd, m, r, s)
        elif self.pix_fmt is None:
            rc = lib.avx_i420_to_rgb_u8(ctx._h, d_yuv.ptr, d_rgb.ptr, n, H, W, m, r, s)
        else:
            rc = lib.avx_yuv_to_rgb_u8(ctx._h, fmt, d_yuv.ptr, d_rgb.ptr, n, H, W, m, r, s)
        ctx._check(rc)

    def arrays(self, buf: np.ndarray, H: int, W: int, ctx: Optional[Context] = None) -> np.ndarray:
        """Payload(s) -> RGB uint8.  `buf`: uint8 of one frame (any shape holding frame_bytes(H, W) bytes, 16-bit samples as
        little-endian byte pairs) -> (Hd, Wd, 3), or with a leading frame axis (N, frame_bytes) -> (N, Hd, Wd, 3)."""
        Hd, Wd = self.out_hw(H, W)
        fsz = self.frame_bytes(H, W)
        a = np.ascontiguousarray(buf)
        if a.dtype != np.uint8:
            raise TypeError(f"{'I420' if self.pix_fmt is None else 'raw video'} payloads are uint8 (got {a.dtype})")
        batched = a.ndim == 2 and a.shape[1] == fsz
        if not batched and a.size != fsz:
            what = "" if self.pix_fmt is None else f" {self.pix_fmt}"
            raise ValueError(f"expected {fsz} bytes per {H}x{W}{what} frame (or an (N, {fsz}) batch), got shape {a.shape}")
        n = a.shape[0] if batched else 1
        out = _through_device(ctx, a, (n, Hd, Wd, 3), lambda c, d_in, d_out: self.launch(c, d_in, d_out, n, H, W))
        return out if batched else out[0]


@dataclasses.dataclass(frozen=True)
class Encode:
    """How RGB uint8 frames become YUV payloads: pix_fmt None is I420, else one of PIX_FMTS."""
    pix_fmt: Optional[str] = None
    matrix: str = "bt601"
    range: str = "limited"

    def __post_init__(self):
        _codes(self.matrix, self.range)
        if self.pix_fmt is not None:
            _fmt_code(self.pix_fmt)

    def frame_bytes(self, H: int, W: int) -> int:
        """Bytes of one H x W payload."""
        return i420_size(H, W) if self.pix_fmt is None else frame_size(self.pix_fmt, H, W)

    def launch(self, ctx: Context, d_rgb: DeviceBuffer, d_yuv: DeviceBuffer, n_frames: int, H: int, W: int, stream=None) -> None:
        """n_frames RGB frames of H x W in d_rgb -> n_frames payloads in d_yuv: every check, then one launch."""
        _check_sizes(n_frames, H, W, d_rgb, d_yuv, self.pix_fmt)
        m, r, n, H, W, s = MATRICES[self.matrix], RANGES[self.range], int(n_frames), int(H), int(W), ctx._s(stream)
        if self.pix_fmt is None:
            rc = lib.avx_rgb_to_i420_u8(ctx._h, d_rgb.ptr, d_yuv.ptr, n, H, W, m, r, s)
        else:
            rc = lib.avx_rgb_to_yuv_u8(ctx._h, AVX_PIX_FMTS[self.pix_fmt], d_rgb.ptr, d_yuv.ptr, n, H, W, m, r, s)
        ctx._check(rc)

    def arrays(self, rgb: np.ndarray, ctx: Optional[Context] = None) -> np.ndarray:
        """RGB uint8 (H, W, 3) -> flat uint8 payload (frame_bytes(H, W),), or (N, H, W, 3) -> (N, frame_bytes(H, W))."""
        a = np.ascontiguousarray(rgb)
        if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
            raise ValueError(f"expected uint8 (H, W, 3) or (N, H, W, 3), got {a.dtype} {a.shape}")
        batched = a.ndim == 4
        n, H, W = (a.shape[0] if batched else 1), a.shape[-3], a.shape[-2]
        out = _through_device(ctx, a, (n, self.frame_bytes(H, W)), lambda c, d_in, d_out: self.launch(c, d_in, d_out, n, H, W))
        return out if batched else out[0]


def codec(pix_fmt: Optional[str] = None, matrix: str = "bt601", range: str = "limited", transfer: Optional[str] = None,
          tonemap: str = "mobius", peak_nits: float = 1000.0, sdr_white: float = 203.0, out_matrix: Optional[str] = None,
          scale: Optional[Tuple[int, int]] = None) -> Tuple[Decode, Encode]:
    """The (Decode, Encode) of a stream that is read and written in one format, from the keywords FramePipeline and VideoRenderer
    take.  The output side is SDR: its matrix is `out_matrix`, which defaults to "bt709" with a transfer and to `matrix` without."""
    decode = Decode(pix_fmt, matrix, range, transfer, tonemap, peak_nits, sdr_white, scale)
    return decode, Encode(pix_fmt, out_matrix or ("bt709" if transfer is not None else matrix), range)


# ---------------------------------------------------------------- the I420 pair of the Y4M path (csrc/yuv.hip) ---------------------
def i420_to_rgb_device(ctx: Context, d_yuv: DeviceBuffer, d_rgb: DeviceBuffer, n_frames: int, H: int, W: int, *, matrix: str = "bt601",
                       range: str = "limited", stream=None) -> None:
    Decode(None, matrix, range).launch(ctx, d_yuv, d_rgb, n_frames, H, W, stream)


def rgb_to_i420_device(ctx: Context, d_rgb: DeviceBuffer, d_yuv: DeviceBuffer, n_frames: int, H: int, W: int, *, matrix: str = "bt601",
                       range: str = "limited", stream=None) -> None:
    Encode(None, matrix, range).launch(ctx, d_rgb, d_yuv, n_frames, H, W, stream)


def i420_to_rgb(buf: np.ndarray, H: int, W: int, *, matrix: str = "bt601", range: str = "limited", ctx: Optional[Context] = None) -> np.ndarray:
    """I420 payload(s) -> RGB uint8.  `buf`: uint8 of one frame (any shape holding i420_size(H, W) bytes, e.g. flat) -> (H, W, 3),
    or with a leading frame axis (N, i420_size) -> (N, H, W, 3)."""
    return Decode(None, matrix, range).arrays(buf, H, W, ctx)


def rgb_to_i420(rgb: np.ndarray, *, matrix: str = "bt601", range: str = "limited", ctx: Optional[Context] = None) -> np.ndarray:
    """RGB uint8 (H, W, 3) -> flat I420 payload (i420_size(H, W),), or (N, H, W, 3) -> (N, i420_size(H, W))."""
    return Encode(None, matrix, range).arrays(rgb, ctx)


# ---------------------------------------------------------------- raw pixel formats (csrc/yuv_raw.hip) ---------------------------
# A format name is required below: None, which a Decode or an Encode reads as I420, is refused first (_fmt_code).
def yuv_to_rgb_device(ctx: Context, pix_fmt: str, d_yuv: DeviceBuffer, d_rgb: DeviceBuffer, n_frames: int, H: int, W: int, *,
                      matrix: str = "bt601", range: str = "limited", stream=None) -> None:
    _fmt_code(pix_fmt)
    Decode(pix_fmt, matrix, range).launch(ctx, d_yuv, d_rgb, n_frames, H, W, stream)


def rgb_to_yuv_device(ctx: Context, pix_fmt: str, d_rgb: DeviceBuffer, d_yuv: DeviceBuffer, n_frames: int, H: int, W: int, *,
                      matrix: str = "bt601", range: str = "limited", stream=None) -> None:
    _fmt_code(pix_fmt)
    Encode(pix_fmt, matrix, range).launch(ctx, d_rgb, d_yuv, n_frames, H, W, stream)


def yuv_to_rgb(buf: np.ndarray, H: int, W: int, *, pix_fmt: str, matrix: str = "bt601", range: str = "limited",
               ctx: Optional[Context] = None) -> np.ndarray:
    """Raw payload(s) in `pix_fmt` -> RGB uint8.  `buf`: uint8 of one frame (frame_size(pix_fmt, H, W) bytes, 16-bit samples as
    little-endian byte pairs) -> (H, W, 3), or with a leading frame axis (N, frame_size) -> (N, H, W, 3)."""
    _fmt_code(pix_fmt)
    return Decode(pix_fmt, matrix, range).arrays(buf, H, W, ctx)


def rgb_to_yuv(rgb: np.ndarray, *, pix_fmt: str, matrix: str = "bt601", range: str = "limited", ctx: Optional[Context] = None) -> np.ndarray:
    """RGB uint8 (H, W, 3) -> flat uint8 payload in `pix_fmt` (frame_size bytes), or (N, H, W, 3) -> (N, frame_size)."""
    _fmt_code(pix_fmt)
    return Encode(pix_fmt, matrix, range).arrays(rgb, ctx)


# ---------------------------------------------------------------- HDR in: PQ / HLG BT.2020 -> SDR RGB (csrc/yuv_hdr.hip) ----------
def _hdr_decode(pix_fmt, transfer, range, tonemap, peak_nits, sdr_white, scale=None) -> Decode:
    """The Decode of the HDR functions below.  A transfer is required there: None, which a Decode reads as SDR, is refused first."""
    hdr_codes(pix_fmt, transfer, range, tonemap, peak_nits, sdr_white)
    return Decode(pix_fmt, "bt601", range, transfer, tonemap, peak_nits, sdr_white, scale)


def yuv_hdr_to_rgb_device(ctx: Context, pix_fmt: str, d_yuv: DeviceBuffer, d_rgb: DeviceBuffer, n_frames: int, H: int, W: int, *,
                          transfer: str, range: str = "limited", tonemap: str = "mobius", peak_nits: float = 1000.0,
                          sdr_white: float = 203.0, stream=None) -> None:
    """n_frames 10-bit BT.2020 payloads in `pix_fmt` with the `transfer` curve -> tone-mapped sRGB uint8 frames."""
    _hdr_decode(pix_fmt, transfer, range, tonemap, peak_nits, sdr_white).launch(ctx, d_yuv, d_rgb, n_frames, H, W, stream)


def yuv_hdr_to_rgb(buf: np.ndarray, H: int, W: int, *, pix_fmt: str, transfer: str, range: str = "limited", tonemap: str = "mobius",
                   peak_nits: float = 1000.0, sdr_white: float = 203.0, ctx: Optional[Context] = None) -> np.ndarray:
    """HDR payload(s) -> SDR RGB uint8, with the payload and batch conventions of yuv_to_rgb: one frame (frame_size(pix_fmt, H, W)
    bytes) -> (H, W, 3), or (N, frame_size) -> (N, H, W, 3)."""
    return _hdr_decode(pix_fmt, transfer, range, tonemap, peak_nits, sdr_white).arrays(buf, H, W, ctx)


# ---------------------------------------------------------------- scaled decode: YUV -> RGB at a smaller size (csrc/yuv_scale.hip) --
def yuv_to_rgb_scaled_device(ctx: Context, pix_fmt: str, d_yuv: DeviceBuffer, d_rgb: DeviceBuffer, n_frames: int, H: int, W: int, Hd: int,
                             Wd: int, *, matrix: str = "bt601", range: str = "limited", stream=None) -> None:
    """n_frames payloads of H x W in `pix_fmt` -> n_frames RGB uint8 frames of Hd x Wd, in one launch: byte for byte
    yuv_to_rgb_device followed by geometry.resize(..., INTER_AREA) per frame."""
    _fmt_code(pix_fmt)
    Decode(pix_fmt, matrix, range, scale=(Wd, Hd)).launch(ctx, d_yuv, d_rgb, n_frames, H, W, stream)


def yuv_to_rgb_scaled(buf: np.ndarray, H: int, W: int, Hd: int, Wd: int, *, pix_fmt: str, matrix: str = "bt601", range: str = "limited",
                      ctx: Optional[Context] = None) -> np.ndarray:
    """Raw payload(s) of H x W in `pix_fmt` -> RGB uint8 of Hd x Wd, with the payload and batch conventions of yuv_to_rgb: one frame
    -> (Hd, Wd, 3), or (N, frame_size) -> (N, Hd, Wd, 3)."""
    _fmt_code(pix_fmt)
    return Decode(pix_fmt, matrix, range, scale=(Wd, Hd)).arrays(buf, H, W, ctx)


# ---------------------------------------------------------------- scaled HDR decode (csrc/yuv_hdr_scale.hip) -----------------------
def yuv_hdr_to_rgb_scaled_device(ctx: Context, pix_fmt: str, d_yuv: DeviceBuffer, d_rgb: DeviceBuffer, n_frames: int, H: int, W: int, Hd: int,
                                 Wd: int, *, transfer: str, range: str = "limited", tonemap: str = "mobius", peak_nits: float = 1000.0,
                                 sdr_white: float = 203.0, stream=None) -> None:
    """n_frames 10-bit BT.2020 payloads of H x W in `pix_fmt` with the `transfer` curve -> n_frames tone-mapped sRGB uint8 frames of
    Hd x Wd, in one launch: byte for byte yuv_hdr_to_rgb_device followed by geometry.resize(..., INTER_AREA) per frame."""
    _hdr_decode(pix_fmt, transfer, range, tonemap, peak_nits, sdr_white, (Wd, Hd)).launch(ctx, d_yuv, d_rgb, n_frames, H, W, stream)


def yuv_hdr_to_rgb_scaled(buf: np.ndarray, H: int, W: int, Hd: int, Wd: int, *, pix_fmt: str, transfer: str, range: str = "limited",
                          tonemap: str = "mobius", peak_nits: float = 1000.0, sdr_white: float = 203.0,
                          ctx: Optional[Context] = None) -> np.ndarray:
    """HDR payload(s) of H x W -> SDR RGB uint8 of Hd x Wd, with the payload and batch conventions of yuv_to_rgb: one frame ->
    (Hd, Wd, 3), or (N, frame_size) -> (N, Hd, Wd, 3)."""
    return _hdr_decode(pix_fmt, transfer, range, tonemap, peak_nits, sdr_white, (Wd, Hd)).arrays(buf, H, W, ctx)
