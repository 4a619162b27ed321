"""NumPy restatement of the raw pixel format arithmetic of DESIGN §4.9 (csrc/yuv_raw.hip), written from the definition alone.

int32 fixed point with 16 fractional bits; coefficients round(c * 2^16), half away from zero, from float64.  For bit depth d:
s = 2^(d-8), chroma centre c = 2^(d-1); limited range (yo, ys, cs) = (16 s, 219 s / 255, 224 s / 255), full range
(0, (2^d - 1) / 255, (2^d - 1) / 255)."""
import numpy as np

KRKB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}

# name: (log2 horizontal subsampling, log2 vertical subsampling, chroma interleaved, bit depth, sample shift, luma only)
FORMATS = {
    "yuv420p": (1, 1, False, 8, 0, False),
    "nv12": (1, 1, True, 8, 0, False),
    "yuv422p": (1, 0, False, 8, 0, False),
    "yuv444p": (0, 0, False, 8, 0, False),
    "gray": (0, 0, False, 8, 0, True),
    "yuv420p10le": (1, 1, False, 10, 0, False),
    "yuv422p10le": (1, 0, False, 10, 0, False),
    "yuv444p10le": (0, 0, False, 10, 0, False),
    "p010le": (1, 1, True, 10, 6, False),
}
COMBOS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]


def q16(c: float) -> int:
    return int(np.sign(c) * np.floor(abs(c) * 65536.0 + 0.5))


def depth_of(fmt: str) -> int:
    return FORMATS[fmt][3]


def range_params(rng: str, d: int):
    """(Y offset, luma scale, chroma scale) at bit depth d."""
    s, top = 2 ** (d - 8), 2 ** d - 1
    return (16 * s, 219 * s / 255.0, 224 * s / 255.0) if rng == "limited" else (0, top / 255.0, top / 255.0)


def dec_coef(matrix: str, rng: str, d: int):
    """(cy, crv, cgu, cgv, cbu, yo): R = cy y + crv v, G = cy y + cgu u + cgv v, B = cy y + cbu u."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    yo, ys, cs = range_params(rng, d)
    return (q16(1.0 / ys), q16(2 * (1 - kr) / cs), q16(-2 * kb * (1 - kb) / (kg * cs)), q16(-2 * kr * (1 - kr) / (kg * cs)),
            q16(2 * (1 - kb) / cs), yo)


def enc_coef(matrix: str, rng: str, d: int):
    """Rows (Y, U, V) of (r, g, b) coefficients, and the Y offset; each row's G coefficient is derived: the Y row sums to
    q16(ys), the chroma rows to 0."""
    kr, kb = KRKB[matrix]
    yo, ys, cs = range_params(rng, d)
    yr, yb = q16(ys * kr), q16(ys * kb)
    ur, ub = q16(-cs * kr / (2 * (1 - kb))), q16(cs * 0.5)
    vr, vb = q16(cs * 0.5), q16(-cs * kb / (2 * (1 - kr)))
    return ((yr, q16(ys) - yr - yb, yb), (ur, -ur - ub, ub), (vr, -vr - vb, vb)), yo


def plane_shapes(fmt: str, H: int, W: int):
    """(chroma rows, chroma columns) of one frame; (0, 0) for a luma-only format."""
    sx, sy, _, _, _, luma = FORMATS[fmt]
    return (0, 0) if luma else (-(-H >> sy), -(-W >> sx))


def frame_size(fmt: str, H: int, W: int) -> int:
    ch, cw = plane_shapes(fmt, H, W)
    return (H * W + 2 * ch * cw) * (2 if depth_of(fmt) > 8 else 1)


def decode_px(Y, U, V, matrix: str, rng: str, d: int):
    """Per-pixel decode of integer sample arrays (any shape) -> R, G, B uint8 arrays."""
    cy, crv, cgu, cgv, cbu, yo = dec_coef(matrix, rng, d)
    Y, u, v = (np.asarray(a, np.int64) for a in (Y, U, V))
    u, v = u - (1 << (d - 1)), v - (1 << (d - 1))
    ly = cy * (Y - yo) + (1 << 15)
    f = lambda a: np.clip(a >> 16, 0, 255).astype(np.uint8)  # noqa: E731
    return f(ly + crv * v), f(ly + cgu * u + cgv * v), f(ly + cbu * u)


def _samples(a: np.ndarray, fmt: str) -> np.ndarray:
    """(N, frame bytes) uint8 -> (N, samples) integer sample values (16-bit samples little-endian, shifted down)."""
    d, sh = FORMATS[fmt][3], FORMATS[fmt][4]
    if d == 8:
        return a.astype(np.int64)
    return ((a[:, 0::2].astype(np.int64) | (a[:, 1::2].astype(np.int64) << 8)) >> sh)


def _bytes(v: np.ndarray, fmt: str) -> np.ndarray:
    """(N, samples) integer sample values -> (N, frame bytes) uint8."""
    d, sh = FORMATS[fmt][3], FORMATS[fmt][4]
    if d == 8:
        return v.astype(np.uint8)
    w = v.astype(np.int64) << sh
    out = np.empty((v.shape[0], 2 * v.shape[1]), np.uint8)
    out[:, 0::2], out[:, 1::2] = w & 255, w >> 8
    return out


def split_planes(yuv: np.ndarray, fmt: str, H: int, W: int):
    """(N, frame bytes) -> integer sample planes Y (N, H, W), U, V (N, ch, cw); U = V = None for a luma-only format."""
    il = FORMATS[fmt][2]
    ch, cw = plane_shapes(fmt, H, W)
    s = _samples(np.asarray(yuv, np.uint8).reshape(-1, frame_size(fmt, H, W)), fmt)
    Y = s[:, : H * W].reshape(-1, H, W)
    if ch == 0:
        return Y, None, None
    c = s[:, H * W:]
    if il:
        c = c.reshape(-1, ch, cw, 2)
        return Y, c[..., 0], c[..., 1]
    return Y, c[:, : ch * cw].reshape(-1, ch, cw), c[:, ch * cw:].reshape(-1, ch, cw)


def join_planes(Y, U, V, fmt: str) -> np.ndarray:
    """The inverse of split_planes: -> (N, frame bytes) uint8."""
    N = Y.shape[0]
    parts = [Y.reshape(N, -1)]
    if U is not None:
        parts += [np.stack([U, V], axis=-1).reshape(N, -1)] if FORMATS[fmt][2] else [U.reshape(N, -1), V.reshape(N, -1)]
    return _bytes(np.concatenate(parts, axis=1), fmt)


def decode(yuv: np.ndarray, fmt: str, H: int, W: int, matrix: str = "bt601", rng: str = "limited") -> np.ndarray:
    """(N, frame_size) or flat one-frame payload -> (N, H, W, 3) / (H, W, 3); chroma replicated over its block."""
    sx, sy, _, d, _, _ = FORMATS[fmt]
    one = np.asarray(yuv).ndim == 1
    Y, U, V = split_planes(yuv, fmt, H, W)
    if U is None:
        U = V = np.full_like(Y, 1 << (d - 1))
    else:
        U, V = (p.repeat(1 << sy, 1).repeat(1 << sx, 2)[:, :H, :W] for p in (U, V))
    out = np.stack(decode_px(Y, U, V, matrix, rng, d), axis=-1)
    return out[0] if one else out


def encode(rgb: np.ndarray, fmt: str, matrix: str = "bt601", rng: str = "limited") -> np.ndarray:
    """(N, H, W, 3) / (H, W, 3) uint8 -> (N, frame_size) / flat payload; an odd last row / column is replicated into its block."""
    sx, sy, _, d, _, luma = FORMATS[fmt]
    a = np.asarray(rgb, np.uint8)
    one = a.ndim == 3
    a = a.reshape((-1,) + a.shape[-3:]).astype(np.int64)
    N, H, W, _ = a.shape
    (ry, ru, rv), yo = enc_coef(matrix, rng, d)
    top, c, lg = (1 << d) - 1, 1 << (d - 1), sx + sy
    Y = np.clip(((a @ np.array(ry, np.int64) + (1 << 15)) >> 16) + yo, 0, top)
    U = V = None
    if not luma:
        bh, bw = 1 << sy, 1 << sx
        p = np.pad(a, ((0, 0), (0, -H % bh), (0, -W % bw), (0, 0)), mode="edge")
        S = sum(p[:, dy::bh, dx::bw] for dy in range(bh) for dx in range(bw))
        U = np.clip(c + ((S @ np.array(ru, np.int64) + (1 << (15 + lg))) >> (16 + lg)), 0, top)
        V = np.clip(c + ((S @ np.array(rv, np.int64) + (1 << (15 + lg))) >> (16 + lg)), 0, top)
    out = join_planes(Y, U, V, fmt)
    return out[0] if one else out


def decode_float(Y, U, V, matrix: str, rng: str, d: int):
    """The float64 formula the fixed point approximates: R, G, B (0..255 scale) before rounding and clamping."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    yo, ys, cs = range_params(rng, d)
    c = 1 << (d - 1)
    y = (np.asarray(Y, np.float64) - yo) / ys
    pb, pr = (np.asarray(U, np.float64) - c) / cs, (np.asarray(V, np.float64) - c) / cs
    return y + 2 * (1 - kr) * pr, y - 2 * kb * (1 - kb) / kg * pb - 2 * kr * (1 - kr) / kg * pr, y + 2 * (1 - kb) * pb


def encode_float(R, G, B, matrix: str, rng: str, d: int):
    """The float64 encode of one pixel (n = 1 block): Y, U, V before rounding and clamping."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    yo, ys, cs = range_params(rng, d)
    R, G, B = (np.asarray(x, np.float64) for x in (R, G, B))
    yl = kr * R + kg * G + kb * B
    return yo + ys * yl, (1 << (d - 1)) + cs * (B - yl) / (2 * (1 - kb)), (1 << (d - 1)) + cs * (R - yl) / (2 * (1 - kr))


def random_payload(fmt: str, n: int, H: int, W: int, seed: int) -> np.ndarray:
    """(n, frame_size) payloads of valid samples: every 8-bit code, 0..1023 at 10 bits; p010le's low 6 bits are random, because
    a reader must ignore them."""
    d, sh = FORMATS[fmt][3], FORMATS[fmt][4]
    g = np.random.default_rng(seed)
    ns = frame_size(fmt, H, W) // (2 if d > 8 else 1)
    out = _bytes(g.integers(0, 1 << d, (n, ns)), fmt)
    if sh:
        out[:, 0::2] |= g.integers(0, 1 << sh, (n, ns)).astype(np.uint8)
    return out
