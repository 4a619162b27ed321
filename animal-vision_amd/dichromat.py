"""Host logic of the dichromat path: 3x3 collapse matrix, OpenCV-style tap generation, and the
DichromatOp that drives the fused HIP kernel (csrc/dichromat.hip) through the C ABI.

Mirrors the per-species template of the reference (animals/dog.py:14-61 and 19 siblings):
validate -> normalise -> sRGB->linear -> collapse matrix -> post stage -> OETF -> dtype restore.
Everything per-pixel runs on the device; only 9-element matrices and <=33 taps are built here."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import DichromatDesc, lib
from .runtime import Context, DeviceBuffer, get_context

# animals/animal_utils.py:56-63 (float32) and :70-76 (float64: the literal has no dtype)
M_RGB_TO_LMS = np.array(
    [[0.31399022, 0.63951294, 0.04649755], [0.15537241, 0.75789446, 0.08670142], [0.01775239, 0.10944209, 0.87256922]],
    dtype=np.float32,
)
M_LMS_TO_RGB = np.array(
    [[5.472213, -4.6419606, 0.16963711], [-1.125242, 2.2931712, -0.16789523], [0.02980164, -0.19318072, 1.1636479]]
)


def collapse_LMS_matrix(alpha: float, s_scale: float) -> np.ndarray:
    """animals/animal_utils.py:88-119.  T = float32(LMS(E) @ D.T @ M_lms_to_rgb.T); callers apply it
    as `pixels @ T.T`, i.e. out_i = sum_j T[i][j] * in_j -- exactly how the kernel consumes it (Q1)."""
    E = np.eye(3, dtype=np.float32)
    LMS = E @ M_RGB_TO_LMS.T
    D = np.array([[alpha, 1.0 - alpha, 0.0], [alpha, 1.0 - alpha, 0.0], [0.0, 0.0, s_scale]], dtype=np.float32)
    return ((LMS @ D.T) @ M_LMS_TO_RGB.T).astype(np.float32)


def cv_auto_ksize(sigma: float) -> int:
    """OpenCV createGaussianKernels for non-uint8 depth and ksize=(0,0): cvRound(8*sigma+1)|1
    (what cv2.GaussianBlur(img, (0,0), sigma) resolves to in animals/animal_utils.py:144)."""
    return int(round(sigma * 8 + 1)) | 1  # Python round == cvRound (half to even)


def gaussian_taps(ksize: int, sigma: float) -> np.ndarray:
    """cv::getGaussianKernel(ksize, sigma > 0) in double: exp(-x^2/(2 sigma^2)) / sum, summed left to right."""
    scale2x = -0.5 / (sigma * sigma)
    c = (ksize - 1) * 0.5
    t = [math.exp(scale2x * (i - c) * (i - c)) for i in range(ksize)]
    s = 0.0
    for v in t:
        s += v
    s = 1.0 / s
    return np.array([v * s for v in t], dtype=np.float64)


def s_cone_row_gain(H: int, s_top=1.0, s_bottom=0.6, *, power=1.0, extra_boost=0.0, band=None) -> np.ndarray:
    """Per-row gain vector of apply_s_cone_vertical_gain (animals/animal_utils.py:236-250); H floats."""
    w = np.linspace(s_top, s_bottom, H, dtype=np.float32)
    if power != 1.0:
        t = (w - s_bottom) / max(1e-8, (s_top - s_bottom))
        t = np.clip(t, 0.0, 1.0) ** power
        w = s_bottom + (s_top - s_bottom) * t
    if extra_boost != 0.0:
        w = 1.0 + extra_boost * (w - 1.0)
    if band is not None:
        y_center, sigma, peak = band
        yy = np.linspace(0.0, 1.0, H, dtype=np.float32)
        w = w * (1.0 + peak * np.exp(-0.5 * ((yy - y_center) / max(1e-8, sigma)) ** 2))
    return np.ascontiguousarray(w, dtype=np.float32)


STREAK_STRIDE = 48


def streak_row_tables(H: int, y_center: float, sigma_streak: float, sigma_far: float, falloff: float) -> np.ndarray:
    """Per-image-row kernels of apply_anisotropic_acuity_blur_with_streak (animals/animal_utils.py:156-171):
    sigma map :157-162 in float32 exactly as coded, then for each row the two cv2.GaussianBlur kernels
    (ksize (0,0) -> cvRound(8 sigma + 1)|1, getGaussianKernel taps cast to the image's float32).
    Layout per row: [k1, k2, 13 x taps(sigmaX), 33 x taps(sigmaY)]."""
    yy = np.linspace(0, 1, H, dtype=np.float32)[:, None]
    d = np.abs(yy - y_center)
    sigma_map = sigma_streak + (sigma_far - sigma_streak) * (1.0 - np.exp(-falloff * d**2))
    sigmaY = sigma_map
    sigmaX = np.maximum(0.4, 0.5 * sigma_map)
    out = np.zeros((H, STREAK_STRIDE), np.float32)
    cache = {}
    for y in range(H):
        sx, sy = float(sigmaX[y, 0]), float(sigmaY[y, 0])
        key = (sx, sy)
        row = cache.get(key)
        if row is None:
            k1, k2 = cv_auto_ksize(sx), cv_auto_ksize(sy)
            if k1 > 13 or k2 > 33:
                raise ValueError(f"streak sigma too large for the device tables (k1={k1}, k2={k2})")
            row = np.zeros(STREAK_STRIDE, np.float32)
            row[0], row[1] = k1, k2
            row[2 : 2 + k1] = gaussian_taps(k1, sx).astype(np.float32)
            row[15 : 15 + k2] = gaussian_taps(k2, sy).astype(np.float32)
            cache[key] = row
        out[y] = row
    return out


@dataclass
class DichromatSpec:
    """One dichromat species: colour stage + post stage."""

    name: str
    alpha: float
    s_scale: float = 1.0
    color: str = "collapse"      # "collapse": dog.py:46-47 | "cat_merge": cat.py:95-101 (float64 tail)
    post: str = "gauss"          # "gauss" | "scone" | "streak" | "none"
    sigma: float = 0.0
    scone: Tuple[float, float, float, float] = (1.3, 0.5, 1.4, 0.25)  # s_top, s_bottom, power, extra_boost
    streak: Tuple[float, float, float, float] = (0.5, 0.8, 2.2, 6.0)
    chroma: Optional[float] = None   # apply_chroma_compression strength whose result is USED
    

ROD_SIGMA, BLOOM_SIGMA = 1.2, 3.0  # apply_rod_vision's and apply_tapetum_bloom's blurs (animal_utils.py:261-305, :183-204): fixed


@dataclass(frozen=True)
class NightSpec:
    """A dichromat at night: apply_rod_vision in front of the colour stage with the values of the reference's
    commented call (animals/cat.py:50-60), and apply_tapetum_bloom behind the post stage when `bloom` (its strength) is above 0."""

    chroma_scale: float = 0.07
    luminance_boost: float = 1.8
    gamma: float = 0.7
    bloom: float = 0.0

    def __post_init__(self):
        for name in ("chroma_scale", "luminance_boost", "gamma", "bloom"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"NightSpec.{name} must be a finite number (got {v!r})")
        if not 0.0 <= self.chroma_scale <= 1.0:
            raise ValueError(f"NightSpec.chroma_scale must be in [0, 1] (got {self.chroma_scale})")
        if not self.luminance_boost > 0.0:
            raise ValueError(f"NightSpec.luminance_boost must be positive (got {self.luminance_boost})")
        if not self.gamma > 0.0:
            raise ValueError(f"NightSpec.gamma must be positive (got {self.gamma})")
        if not 0.0 <= self.bloom <= 1.0:
            raise ValueError(f"NightSpec.bloom must be in [0, 1] (got {self.bloom})")


def night_desc(night: NightSpec):
    """(avx_night_desc, the tap arrays it points into) for `night`."""
    rod = gaussian_taps(cv_auto_ksize(ROD_SIGMA), ROD_SIGMA)
    bloom = gaussian_taps(cv_auto_ksize(BLOOM_SIGMA), BLOOM_SIGMA)
    nd = _lib.NightDesc()
    nd.struct_size = ctypes.sizeof(_lib.NightDesc)
    nd.chroma_scale, nd.luminance_boost, nd.gamma = float(night.chroma_scale), float(night.luminance_boost), float(night.gamma)
    nd.rod_ksize = rod.size
    nd.rod_taps_host = rod.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    nd.bloom_strength = float(night.bloom)
    nd.bloom_ksize = bloom.size
    nd.bloom_taps_host = bloom.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    return nd, (rod, bloom)


@dataclass(frozen=True)
class FovSpec:
    """A dichromat's field of view: the binocular wide view of the reference (animal_fov_binocular_warp,
    animals/cat_widevision_utils.py:46-99) in front of the species' colour stage, and the centre-zoomed input
    (zoom_scale_from_cat_ratio, center_zoom) as the baseline.  Each eye sees `per_eye_half_fov_deg` (phi) to either side of its
    axis, the two fields share `overlap_deg` (O), and the camera's frame covers `camera_hfov_deg` (2 psi) of the 4 phi - O degrees
    shown.  The defaults of the last two are Cat's class constants.  The values are the user's: there is no per-species table."""

    per_eye_half_fov_deg: float
    overlap_deg: float
    camera_hfov_deg: float = 100.0
    to_human_ratio: float = 1.30

    def __post_init__(self):
        for name in ("per_eye_half_fov_deg", "overlap_deg", "camera_hfov_deg", "to_human_ratio"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"FovSpec.{name} must be a finite number (got {v!r})")
        if not 0.0 < self.per_eye_half_fov_deg <= 180.0:  # the model divides by phi
            raise ValueError(f"FovSpec.per_eye_half_fov_deg must be above 0 and at most 180 (got {self.per_eye_half_fov_deg})")
        if not 0.0 <= self.overlap_deg <= 360.0:  # alpha = max(0, phi - O / 2)
            raise ValueError(f"FovSpec.overlap_deg must be in [0, 360] (got {self.overlap_deg})")
        if not 0.0 < self.camera_hfov_deg < 180.0:  # the model takes tan(psi) and divides by psi
            raise ValueError(f"FovSpec.camera_hfov_deg must be above 0 and below 180 (got {self.camera_hfov_deg})")
        if not self.to_human_ratio >= 1.0:  # (the reference clamps at 1.01 itself)
            raise ValueError(f"FovSpec.to_human_ratio must be at least 1 (got {self.to_human_ratio})")

    @property
    def shown_deg(self) -> float:
        """The field the output's columns span, in degrees: 4 phi - O (2 phi + 2 alpha, alpha clamped at 0)."""
        return 2.0 * self.per_eye_half_fov_deg + 2.0 * max(0.0, self.per_eye_half_fov_deg - 0.5 * self.overlap_deg)


def as_fov(fov) -> Optional["FovSpec"]:
    """None, a FovSpec, or the arguments of one as a tuple or list (phi, O[, camera[, ratio]])."""
    if fov is None or isinstance(fov, FovSpec):
        return fov
    if isinstance(fov, (tuple, list)) and 2 <= len(fov) <= 4:
        return FovSpec(*fov)
    raise TypeError(f"fov must be None, a FovSpec or its arguments as a tuple (got {type(fov).__name__})")


NIGHT_THRESHOLD = 0.12  # RatUV._choose_mode (animals/rat_uv.py:99-104): night when the median Rec.709 luma is below it


@dataclass(frozen=True)
class AutoNight:
    """Day or night, decided per frame: a frame whose median Rec.709 luma is below `threshold` is shown as `night`
    describes, every other frame by day.  Accepted wherever `night=` takes a NightSpec."""

    night: NightSpec = NightSpec()
    threshold: float = NIGHT_THRESHOLD

    def __post_init__(self):
        if not isinstance(self.night, NightSpec):
            raise TypeError(f"AutoNight.night must be a NightSpec (got {type(self.night).__name__})")
        check_threshold(self.threshold, "AutoNight.threshold")


def check_threshold(v, what: str = "threshold") -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"{what} must be a finite number (got {v!r})")
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{what} must be in [0, 1] (got {v})")
    return float(v)


LUMA_WEIGHTS = (0.2126, 0.7152, 0.0722)


def luma_tables() -> np.ndarray:
    """float32 [3][256]: t_c[v] = w_c * (v / 255) as NumPy forms it on a uint8 frame (oracle NumpyProbes.median_luma), so that
    Y = (t_0[R] + t_1[G]) + t_2[B].  The library computes the same bits (avx_get_table(3))."""
    x = np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0
    return np.stack([w * x for w in LUMA_WEIGHTS]).astype(np.float32, copy=False)


def finish_modes(below, max_below, min_at_or_above, n: int, threshold: float) -> np.ndarray:
    """bool[N]: whether float(np.median(Y)) < threshold, from the records of avx_luma_mode_u8 over frames of n pixels.  The count
    decides unless it is exactly n / 2; then the two middle values are max_below and min_at_or_above, and np.median is their
    float32 mean."""
    below = np.atleast_1d(np.asarray(below)).astype(np.int64)
    a = np.atleast_1d(np.asarray(max_below, np.float32))
    b = np.atleast_1d(np.asarray(min_at_or_above, np.float32))
    out = 2 * below > n
    for f in np.nonzero(2 * below == n)[0]:
        out[f] = float(np.float32(a[f] + b[f]) / np.float32(2)) < threshold
    return out


def luma_records_device(ctx: Context, ptr: int, n_frames: int, H: int, W: int, threshold: float, d_rec: DeviceBuffer, out: Optional[np.ndarray] = None,
                        stream=None) -> np.ndarray:
    """avx_luma_mode_u8 on n_frames (1..16) uint8 frames at device address `ptr`, the records through d_rec (at least 16 bytes per
    frame) into `out` (a structured array of _lib.LUMA_MODE_REC_DTYPE; pinned memory makes the copy asynchronous until the
    synchronisation of `stream` that ends this call)."""
    ctx._check(lib.avx_luma_mode_u8(ctx._h, ptr, n_frames, H, W, float(threshold), d_rec.ptr, ctx._s(stream)))
    if out is None:
        out = np.empty(n_frames, _lib.LUMA_MODE_REC_DTYPE)
    return ctx.download(d_rec, (n_frames,), out.dtype, out=out, stream=stream)[:n_frames]


def luma_modes(frames: np.ndarray, threshold: float = NIGHT_THRESHOLD, ctx: Optional[Context] = None):
    """(night bool[N], below uint32[N], max_below float32[N], min_at_or_above float32[N]) of uint8 host frames N x H x W x 3 or
    H x W x 3: the day/night decision of AutoNight and the record it rests on (avx_luma_mode_u8; max_below is 0 where below is 0,
    min_at_or_above +inf where every pixel is below)."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        raise NotImplementedError(f"luma_modes takes uint8 frames (got {frames.dtype})")
    batch = frames[None] if frames.ndim == 3 else frames
    if batch.ndim != 4 or batch.shape[3] != 3 or batch.shape[0] < 1:
        raise ValueError(f"luma_modes takes N x H x W x 3 or H x W x 3 frames (got shape {frames.shape})")
    threshold = check_threshold(threshold)
    ctx = ctx or get_context()
    N, H, W, _ = batch.shape
    d_in, d_rec = ctx.upload(batch), ctx.malloc(16 * 16)
    try:
        recs = [luma_records_device(ctx, d_in.ptr + f0 * H * W * 3, min(16, N - f0), H, W, threshold, d_rec).copy() for f0 in range(0, N, 16)]
    finally:
        d_in.free()
        d_rec.free()
    rec = np.concatenate(recs)
    return finish_modes(rec["below"], rec["max_below"], rec["min_at_or_above"], H * W, threshold), rec["below"], rec["max_below"], rec["min_at_or_above"]


class DichromatOp:
    """Configured fused kernel launch for one species; reusable across frames (stateless between them).  With `night` (a NightSpec)
    run_device and __call__ go to avx_dichromat_night_u8 (csrc/night.hip) instead of the day kernel; with an AutoNight to
    avx_dichromat_auto_u8 (csrc/daynight.hip), which decides per frame: `last_modes` then holds the last call's decisions
    (uint8, 1 = night) and `auto_counts` [night frames, frames] over the op's life."""

    def __init__(self, spec: DichromatSpec, ctx: Optional[Context] = None, night=None):
        self.spec = spec
        self.ctx = ctx
        if night is not None and not isinstance(night, (NightSpec, AutoNight)):
            raise TypeError(f"night must be a NightSpec, an AutoNight or None (got {type(night).__name__})")
        self.night = night
        self.auto = night if isinstance(night, AutoNight) else None
        night = night.night if self.auto is not None else night
        self.last_modes = np.zeros(0, np.uint8)
        self.auto_counts = [0, 0]
        self.night_desc, self._night_taps = night_desc(night) if night is not None else (None, None)
        d = DichromatDesc()
        d.struct_size = ctypes.sizeof(DichromatDesc)
        if spec.color == "collapse":
            d.color_mode = _lib.AVX_COLOR_MATRIX
            T = collapse_LMS_matrix(spec.alpha, spec.s_scale)
            d.matrix = (ctypes.c_float * 9)(*T.reshape(-1).tolist())
        elif spec.color == "cat_merge":
            d.color_mode = _lib.AVX_COLOR_CAT_MERGE
            d.cat_alpha = float(np.float32(spec.alpha))
            d.cat_beta = float(np.float32(1.0 - spec.alpha))
        else:
            raise ValueError(f"unknown colour stage {spec.color!r}")
        self._taps = None
        self._gain = None
        if spec.post == "gauss":
            k = cv_auto_ksize(spec.sigma)
            if k > _lib.AVX_MAX_KSIZE:
                raise ValueError(f"sigma {spec.sigma} needs {k} taps > {_lib.AVX_MAX_KSIZE}")
            self._taps = gaussian_taps(k, spec.sigma)
            d.post_mode = _lib.AVX_POST_GAUSS
            d.ksize = k
            d.taps_host = self._taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        elif spec.post == "scone":
            d.post_mode = _lib.AVX_POST_ROWGAIN
            d.row_gain_clamp = 1
        elif spec.post == "streak":
            if spec.color != "collapse":
                raise ValueError("the streak blur runs on the float32 collapse-matrix colour stage")
            d.post_mode = _lib.AVX_POST_STREAK
            d.streak_stride = STREAK_STRIDE
        elif spec.post == "none":
            d.post_mode = _lib.AVX_POST_NONE
        else:
            raise ValueError(f"unknown post stage {spec.post!r}")
        self._streak = None
        if spec.chroma is not None:
            d.chroma_enable = 1
            d.chroma_keep = float(np.float32(1 - spec.chroma))
        self.desc = d

    def _ctx(self) -> Context:
        if self.ctx is None:
            self.ctx = get_context()
        return self.ctx

    def prepare_tables(self, H: int) -> None:
        """The desc's per-row host tables (row gains, streak taps) for frames of H rows; kept until H changes."""
        if self.spec.post == "scone":
            if self._gain is None or self._gain.size != H:
                s_top, s_bottom, power, boost = self.spec.scone
                self._gain = s_cone_row_gain(H, s_top, s_bottom, power=power, extra_boost=boost)
            self.desc.row_gain_host = self._gain.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        if self.spec.post == "streak":
            if self._streak is None or self._streak.shape[0] != H:
                self._streak = streak_row_tables(H, *self.spec.streak)
            self.desc.streak_rows_host = self._streak.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    max_batch = 16  # frames one run_device call takes from a pipeline slot (pipeline.FramePipeline(batch=))

    def run_device(self, d_in: DeviceBuffer, d_out: DeviceBuffer, n_frames: int, H: int, W: int, stream=None):
        """N uint8 HWC frames resident in HBM -> N uint8 HWC frames; asynchronous on `stream`."""
        ctx = self._ctx()
        need = n_frames * H * W * 3
        if d_in.nbytes < need * (4 if self.desc.in_f32 else 1) or d_out.nbytes < need:
            raise ValueError("device buffers smaller than n_frames*H*W*3")
        self.prepare_tables(H)
        if self.auto is not None:
            modes = np.zeros(16, np.uint8)
            ctx._check(lib.avx_dichromat_auto_u8(ctx._h, d_in.ptr, d_out.ptr, n_frames, H, W, ctypes.byref(self.desc), ctypes.byref(self.night_desc),
                                                 float(self.auto.threshold), modes.ctypes.data, ctx._s(stream)))
            self.last_modes = modes[:n_frames].copy()
            self.auto_counts[0] += int(self.last_modes.sum())
            self.auto_counts[1] += n_frames
            return
        if self.night is not None:  # (a frame below 13 x 13 is refused by the library, by name)
            ctx._check(lib.avx_dichromat_night_u8(ctx._h, d_in.ptr, d_out.ptr, n_frames, H, W, ctypes.byref(self.desc),
                                                  ctypes.byref(self.night_desc), ctx._s(stream)))
            return
        ctx._check(lib.avx_dichromat_u8(ctx._h, d_in.ptr, d_out.ptr, n_frames, H, W, ctypes.byref(self.desc), ctx._s(stream)))

    def last_launch(self) -> dict:
        """Which kernel and launch geometry the last dichromat call on this op's context ran (avx_dichromat_last_launch; host
        state only).  `family` is one of "reference", "tiled", "march", "streak" ("none": no launch yet); the other keys are
        the integer fields of avx_dichromat_launch_info."""
        ctx = self._ctx()
        info = _lib.DichromatLaunchInfo()
        info.struct_size = ctypes.sizeof(info)
        ctx._check(lib.avx_dichromat_last_launch(ctx._h, ctypes.byref(info)))
        out = {n: int(getattr(info, n)) for n, _ in info._fields_[2:]}
        out["family"] = _lib.AVX_LAUNCH_FAMILIES[info.family]
        return out

    def __call__(self, image: np.ndarray) -> np.ndarray:
        """uint8 HxWx3 (or NxHxWx3) host frame(s) -> same shape uint8, via upload/kernel/download."""
        if image.dtype != np.uint8:
            raise NotImplementedError("device dichromat path takes uint8 frames (float frames: see animal_utils)")
        batch = image if image.ndim == 4 else image[None]
        n, H, W, _ = batch.shape
        ctx = self._ctx()
        d_in = ctx.upload(batch)
        d_out = ctx.malloc(batch.nbytes)
        try:
            if self.auto is not None and n > self.max_batch:  # the switched entry takes at most max_batch frames
                modes, fb = [], H * W * 3
                for f0 in range(0, n, self.max_batch):
                    m = min(self.max_batch, n - f0)
                    self.run_device(d_in.view(f0 * fb, m * fb), d_out.view(f0 * fb, m * fb), m, H, W)
                    modes.append(self.last_modes)
                self.last_modes = np.concatenate(modes)
            else:
                self.run_device(d_in, d_out, n, H, W)
            out = ctx.download(d_out, batch.shape, np.uint8)
        finally:
            d_in.free()
            d_out.free()
        return out if image.ndim == 4 else out[0]
