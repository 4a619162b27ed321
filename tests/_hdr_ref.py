"""The definition of the HDR decode in float64 NumPy: 10-bit BT.2020 Y'CbCr with a PQ (SMPTE ST 2084) or HLG
(BT.2100) transfer -> tone-mapped SDR sRGB uint8.  Written from the definition alone; csrc/yuv_hdr.hip is held to it within one
output code (tests/test_hdr_host.py for the arithmetic, tests/test_hdr_gpu.py for the kernels).

Steps: Y'CbCr -> R'G'B' (clamped to [0, 1]) -> display light in nits -> v = nits / sdr_white -> all channels times t(m) / m with
m = max(v) -> linear BT.2020 to linear BT.709 in difference form, clamped -> the project's sRGB encoder (the float32 thresholds
of csrc/srgb_tables.h evaluated on the float64 value: code = number of thresholds <= x)."""
import os

import numpy as np

import _rawyuv_ref as R

FORMATS = ("yuv420p10le", "yuv422p10le", "yuv444p10le", "p010le")
TRANSFERS = ("pq", "hlg")
TONEMAPS = ("clip", "mobius")
RANGES = ("limited", "full")
COMBOS = [(t, r, m) for t in TRANSFERS for r in RANGES for m in TONEMAPS]

KR, KB = 0.2627, 0.0593
KG = 1.0 - KR - KB

# SMPTE ST 2084
PQ_M1, PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
PQ_C1, PQ_C2, PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
# BT.2100 HLG
HLG_A = 0.17883277
HLG_B = 1.0 - 4.0 * HLG_A
HLG_C = 0.5 - HLG_A * np.log(4.0 * HLG_A)
HLG_LW, HLG_GAMMA = 1000.0, 1.2
LUM = np.array([0.2627, 0.6780, 0.0593])

KNEE = 0.75

PRIMARIES_2020 = ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))
PRIMARIES_709 = ((0.64, 0.33), (0.30, 0.60), (0.15, 0.06))
D65 = (0.3127, 0.3290)

ENC_THR = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "srgb_tables.npz"))["enc_thr_f32"].astype(np.float64)


def rgb_to_xyz(primaries, white):
    """RGB -> XYZ from chromaticities, as BT.2087 derives it: the primaries' XYZ columns scaled so that (1, 1, 1) is the white."""
    P = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in primaries], np.float64).T
    w = np.array([white[0] / white[1], 1.0, (1.0 - white[0] - white[1]) / white[1]])
    return P * np.linalg.solve(P, w)[None, :]


def gamut_matrix():
    """Linear BT.2020 -> linear BT.709, both at D65."""
    return np.linalg.solve(rgb_to_xyz(PRIMARIES_709, D65), rgb_to_xyz(PRIMARIES_2020, D65))


def ycbcr_to_rgb(Y, U, V, rng: str):
    """10-bit samples -> R', G', B' clamped to [0, 1] (BT.2020 non-constant luminance); arrays of any one shape."""
    Y, U, V = (np.asarray(a, np.float64) for a in (Y, U, V))
    if rng == "limited":
        y, cb, cr = (Y - 64.0) / 876.0, (U - 512.0) / 896.0, (V - 512.0) / 896.0
    else:
        y, cb, cr = Y / 1023.0, (U - 512.0) / 1023.0, (V - 512.0) / 1023.0
    r = y + 2.0 * (1.0 - KR) * cr
    b = y + 2.0 * (1.0 - KB) * cb
    g = y - (2.0 * KB * (1.0 - KB) / KG) * cb - (2.0 * KR * (1.0 - KR) / KG) * cr
    return np.clip(np.stack([r, g, b], -1), 0.0, 1.0)


def pq_eotf(e):
    """E' in [0, 1] -> nits."""
    p = np.asarray(e, np.float64) ** (1.0 / PQ_M2)
    return 10000.0 * (np.maximum(p - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * p)) ** (1.0 / PQ_M1)


def hlg_inverse_oetf(e):
    """E' in [0, 1] -> scene light E in [0, 1]."""
    e = np.asarray(e, np.float64)
    return np.where(e <= 0.5, e * e / 3.0, (np.exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0)


def hlg_to_nits(rgb):
    """(..., 3) E' -> nits: the inverse OETF, then the OOTF at Lw = 1000 nits, gamma 1.2; the factor is 0 at Ys = 0."""
    E = hlg_inverse_oetf(rgb)
    ys = E @ LUM
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(ys > 0.0, ys ** (HLG_GAMMA - 1.0), 0.0)
    return HLG_LW * f[..., None] * E


def to_nits(rgb, transfer: str):
    return pq_eotf(rgb) if transfer == "pq" else hlg_to_nits(rgb)


def tone_curve(m, tonemap: str, P: float):
    """t(m) for m >= 0; P = peak_nits / sdr_white > 1."""
    m = np.asarray(m, np.float64)
    if tonemap == "clip":
        return np.minimum(m, 1.0)
    k = KNEE
    u = (np.minimum(m, P) - k) / (P - k)
    a = (1.0 - k) / (P - 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):  # u + a passes 0 below the knee, where the other branch is taken
        return np.where(m <= k, m, k + (1.0 - k) * u * (1.0 + a) / (u + a))


def tone_map(v, tonemap: str, P: float):
    """(..., 3) -> all three channels times t(m) / m, m their maximum (1 where m = 0)."""
    m = v.max(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(m > 0.0, tone_curve(m, tonemap, P) / m, 1.0)
    return v * s[..., None]


def gamut(x, M=None):
    """(..., 3) linear BT.2020 -> BT.709 in difference form, out_i = x_i + sum_{j != i} M_ij (x_j - x_i); clamped to [0, 1]."""
    M = gamut_matrix() if M is None else M
    out = np.empty_like(x)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        out[..., i] = x[..., i] + (M[i, j] * (x[..., j] - x[..., i]) + M[i, k] * (x[..., k] - x[..., i]))
    return np.clip(out, 0.0, 1.0)


def srgb_encode(x):
    """The project's encoder: the number of thresholds <= x."""
    return np.searchsorted(ENC_THR, np.asarray(x, np.float64), side="right").astype(np.uint8)


def linear_709(Y, U, V, transfer: str, rng: str = "limited", tonemap: str = "mobius", peak_nits: float = 1000.0, sdr_white: float = 203.0):
    """Per-pixel decode up to the encoder's input: (..., 3) float64 in [0, 1]."""
    if not peak_nits > sdr_white > 0:
        raise ValueError("peak_nits > sdr_white > 0 is required")
    v = to_nits(ycbcr_to_rgb(Y, U, V, rng), transfer) / sdr_white
    return gamut(tone_map(v, tonemap, peak_nits / sdr_white))


def decode_px(Y, U, V, transfer: str, rng: str = "limited", tonemap: str = "mobius", peak_nits: float = 1000.0, sdr_white: float = 203.0):
    """Per-pixel decode of integer sample arrays (any one shape) -> (..., 3) uint8."""
    return srgb_encode(linear_709(Y, U, V, transfer, rng, tonemap, peak_nits, sdr_white))


def decode(yuv, fmt: str, H: int, W: int, transfer: str, rng: str = "limited", tonemap: str = "mobius", peak_nits: float = 1000.0,
           sdr_white: float = 203.0):
    """(N, frame_size) or flat one-frame payload -> (N, H, W, 3) / (H, W, 3) uint8; layouts, nearest chroma replication and
    p010le's shift as in tests/_rawyuv_ref.py."""
    if fmt not in FORMATS:
        raise ValueError(f"the HDR decode reads {FORMATS} (got {fmt!r})")
    sx, sy = R.FORMATS[fmt][0], R.FORMATS[fmt][1]
    one = np.asarray(yuv).ndim == 1
    Y, U, V = R.split_planes(yuv, fmt, H, W)
    U, V = (p.repeat(1 << sy, 1).repeat(1 << sx, 2)[:, :H, :W] for p in (U, V))
    out = decode_px(Y, U, V, transfer, rng, tonemap, peak_nits, sdr_white)
    return out[0] if one else out


def lattice():
    """The 11^3 lattice of 10-bit extremes, (1331, 3) of (Y, U, V)."""
    ax = np.array([0, 1, 63, 64, 65, 511, 512, 513, 940, 1022, 1023])
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
