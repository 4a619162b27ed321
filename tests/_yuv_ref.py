"""NumPy restatement of the YUV 4:2:0 <-> RGB arithmetic of DESIGN §4.8 (csrc/yuv.hip), written from the definition alone.

int32 fixed point with 16 fractional bits; coefficients round(c * 2^16) with round half away from zero, from float64."""
import numpy as np

KRKB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def q16(c: float) -> int:
    return int(np.sign(c) * np.floor(abs(c) * 65536.0 + 0.5))


def range_params(rng: str):
    """(Y offset, luma scale, chroma scale)."""
    return (16, 219.0 / 255.0, 224.0 / 255.0) if rng == "limited" else (0, 1.0, 1.0)


def i420_size(H: int, W: int) -> int:
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def dec_coef(matrix: str, rng: str):
    """(cy, crv, cgu, cgv, cbu, yo): R = cy y + crv v, G = cy y + cgu u + cgv v, B = cy y + cbu u."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    yo, ys, cs = range_params(rng)
    return (q16(1.0 / ys), q16(2 * (1 - kr) / cs), q16(-2 * kb * (1 - kb) / (kg * cs)), q16(-2 * kr * (1 - kr) / (kg * cs)),
            q16(2 * (1 - kb) / cs), yo)


def enc_coef(matrix: str, rng: str):
    """Rows (Y, U, V) of (r, g, b) coefficients, and the Y offset; the G coefficient of each row is derived so that the row sums
    to round(ys 2^16) (Y) or 0 (U, V)."""
    kr, kb = KRKB[matrix]
    yo, ys, cs = range_params(rng)
    yr, yb = q16(ys * kr), q16(ys * kb)
    ur, ub = q16(-cs * kr / (2 * (1 - kb))), q16(cs * 0.5)
    vr, vb = q16(cs * 0.5), q16(-cs * kb / (2 * (1 - kr)))
    return ((yr, q16(ys) - yr - yb, yb), (ur, -ur - ub, ub), (vr, -vr - vb, vb)), yo


def decode_px(Y, U, V, matrix, rng):
    """Per-pixel decode of integer arrays (any shape) -> R, G, B uint8 arrays."""
    cy, crv, cgu, cgv, cbu, yo = dec_coef(matrix, rng)
    Y, u, v = (np.asarray(a, np.int64) for a in (Y, U, V))
    u, v = u - 128, v - 128
    ly = cy * (Y - yo) + (1 << 15)
    f = lambda a: np.clip(a >> 16, 0, 255).astype(np.uint8)  # noqa: E731
    return f(ly + crv * v), f(ly + cgu * u + cgv * v), f(ly + cbu * u)


def decode(yuv: np.ndarray, H: int, W: int, matrix: str = "bt601", rng: str = "limited") -> np.ndarray:
    """(N, i420_size) or flat one-frame payload -> (N, H, W, 3) / (H, W, 3)."""
    a = np.asarray(yuv, np.uint8)
    one = a.ndim == 1
    a = a.reshape(-1, i420_size(H, W))
    ch, cw = (H + 1) // 2, (W + 1) // 2
    Y = a[:, : H * W].reshape(-1, H, W)
    U = a[:, H * W: H * W + ch * cw].reshape(-1, ch, cw).repeat(2, 1).repeat(2, 2)[:, :H, :W]
    V = a[:, H * W + ch * cw:].reshape(-1, ch, cw).repeat(2, 1).repeat(2, 2)[:, :H, :W]
    out = np.stack(decode_px(Y, U, V, matrix, rng), axis=-1)
    return out[0] if one else out


def encode(rgb: np.ndarray, matrix: str = "bt601", rng: str = "limited") -> np.ndarray:
    """(N, H, W, 3) / (H, W, 3) uint8 -> (N, i420_size) / flat payload."""
    a = np.asarray(rgb, np.uint8)
    one = a.ndim == 3
    a = a.reshape((-1,) + a.shape[-3:]).astype(np.int64)
    N, H, W, _ = a.shape
    (ry, ru, rv), yo = enc_coef(matrix, rng)
    Y = np.clip(((a @ np.array(ry, np.int64) + (1 << 15)) >> 16) + yo, 0, 255)
    p = np.pad(a, ((0, 0), (0, H % 2), (0, W % 2), (0, 0)), mode="edge")  # an odd last row / column is replicated
    S = p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]
    U = np.clip(128 + ((S @ np.array(ru, np.int64) + (1 << 17)) >> 18), 0, 255)
    V = np.clip(128 + ((S @ np.array(rv, np.int64) + (1 << 17)) >> 18), 0, 255)
    out = np.concatenate([Y.reshape(N, -1), U.reshape(N, -1), V.reshape(N, -1)], axis=1).astype(np.uint8)
    return out[0] if one else out


def decode_float(Y, U, V, matrix: str, rng: str):
    """The float64 formula the fixed point approximates: R, G, B before rounding and clamping."""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    yo, ys, cs = range_params(rng)
    y = (np.asarray(Y, np.float64) - yo) / ys
    pb, pr = (np.asarray(U, np.float64) - 128) / cs, (np.asarray(V, np.float64) - 128) / cs
    return y + 2 * (1 - kr) * pr, y - 2 * kb * (1 - kb) / kg * pb - 2 * kr * (1 - kr) / kg * pr, y + 2 * (1 - kb) * pb


def y4m_bytes(frames, H: int, W: int, header: str = "F30:1 Ip A1:1 C420jpeg", frame_params=None) -> bytes:
    """A .y4m stream of flat payloads; frame_params[k] (str or None) goes after FRAME of frame k."""
    out = [f"YUV4MPEG2 W{W} H{H} {header}\n".encode()]
    for k, f in enumerate(frames):
        p = frame_params[k] if frame_params else None
        out.append(b"FRAME" + (b" " + p.encode() if p else b"") + b"\n")
        out.append(np.asarray(f, np.uint8).tobytes())
    return b"".join(out)
