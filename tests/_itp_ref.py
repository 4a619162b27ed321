"""The definition of dE_ITP (ITU-R BT.2124; DESIGN §4.27, include/avx.h: avx_itp_delta) in float64 NumPy, and a float32 restatement
of the arithmetic that csrc/itp.hip chose for it.

A side is ("sdr", frames) -- uint8 sRGB (N, H, W, 3), BT.709 primaries, code 255 at sdr_white nits -- or ("hdr", payload, fmt,
transfer, rng): (N, frame bytes) of a 10-bit format, BT.2020 Y'CbCr, read as tests/_hdr_ref.py reads it (chroma replicated over its
block, R'G'B' clamped to [0, 1]), display light from its pq_eotf / hlg_to_nits, no tone map.  From nits in BT.2020 RGB: LMS by the
BT.2100 matrix over 4096, L'M'S' by the PQ inverse EOTF of LMS / 10000, I = (L' + M') / 2, Ct and Cp by the BT.2100 rows over 4096,
T = Ct / 2, P = Cp, dE_ITP = 720 sqrt(dI^2 + dT^2 + dP^2).

delta32 restates the kernel in float32, one rounding per operation, with NumPy's float32 log2 / exp2 / division / sqrt where the
device has v_log_f32 / v_exp_f32 / v_rcp_f32 / v_sqrt_f32: what it differs from `delta` by is the cost of float32 in the chosen
form, and the GPU test allows the device eight times that."""
import numpy as np

import _deltae_ref as E
import _rawyuv_ref as R
from _hdr_ref import HLG_A, HLG_B, HLG_C, KB, KG, KR, PQ_C1, PQ_C2, PQ_C3, PQ_M1, PQ_M2, gamut_matrix, hlg_to_nits, pq_eotf, ycbcr_to_rgb

LMS = np.array([[1688.0, 2146.0, 262.0], [683.0, 2951.0, 462.0], [99.0, 309.0, 3688.0]]) / 4096.0
ICTCP = np.array([[2048.0, 2048.0, 0.0], [6610.0, -13613.0, 7003.0], [17933.0, -17390.0, -543.0]]) / 4096.0


def to_2020():
    """Linear BT.709 -> linear BT.2020: the inverse of the HDR decode's matrix; every row sums to 1."""
    return np.linalg.inv(gamut_matrix())


def sdr(frames):
    return ("sdr", np.asarray(frames, np.uint8))


def hdr(payload, fmt, transfer, rng="limited"):
    return ("hdr", np.asarray(payload, np.uint8), fmt, transfer, rng)


def samples(side, H, W):
    """The integer samples of a side per pixel, (N, H, W) each: (r8, g8, b8) or (Y, U, V) with the chroma replicated."""
    if side[0] == "sdr":
        a = side[1].reshape(-1, H, W, 3).astype(np.int64)
        return a[..., 0], a[..., 1], a[..., 2]
    _, payload, fmt, _, _ = side
    sx, sy = R.FORMATS[fmt][0], R.FORMATS[fmt][1]
    Y, U, V = R.split_planes(payload, fmt, H, W)
    U, V = (p.repeat(1 << sy, 1).repeat(1 << sx, 2)[:, :H, :W] for p in (U, V))
    return Y, U, V


# ------------------------------------------------------------------------------------------------ the definition, float64
def pq_inverse(x):
    """nits / 10000 -> E'."""
    p = np.maximum(np.asarray(x, np.float64), 0.0) ** PQ_M1
    return ((PQ_C1 + PQ_C2 * p) / (1.0 + PQ_C3 * p)) ** PQ_M2


def nits_2020(side, H, W, sdr_white=203.0):
    """(N, H, W, 3) display light of a side in BT.2020 RGB, nits."""
    s0, s1, s2 = samples(side, H, W)
    if side[0] == "sdr":
        lin = sdr_white * E.decode_table()[np.stack([s0, s1, s2], -1)]
        g, dr, db = lin[..., 1], lin[..., 0] - lin[..., 1], lin[..., 2] - lin[..., 1]
        N = to_2020()
        return np.stack([g + N[i, 0] * dr + N[i, 2] * db for i in range(3)], -1)
    rgb = ycbcr_to_rgb(s0, s1, s2, side[4])
    return pq_eotf(rgb) if side[3] == "pq" else hlg_to_nits(rgb)


def itp(nits):
    """(..., 3) BT.2020 nits -> (..., 3) of (I, T, P)."""
    lms = pq_inverse(np.asarray(nits, np.float64) @ LMS.T / 10000.0)
    out = lms @ ICTCP.T
    out[..., 1] *= 0.5
    return out


def delta(a, b, H, W, sdr_white=203.0):
    """dE_ITP of two sides, float64 (N, H, W)."""
    d = itp(nits_2020(a, H, W, sdr_white)) - itp(nits_2020(b, H, W, sdr_white))
    return 720.0 * np.sqrt((d * d).sum(-1))


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic, float32
f32 = np.float32
_LOG2E = 1.4426950408889634


def _pw(x, e):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > 0, np.exp2(f32(e) * np.log2(np.where(x > 0, x, f32(1.0)))), f32(0.0)).astype(f32)


def _rcp(x):
    return (f32(1.0) / x).astype(f32)


def _pq_eotf32(e):
    with np.errstate(divide="ignore"):
        t = np.where(e > 0, np.log2(np.where(e > 0, e, f32(1.0))), f32(0.0)).astype(f32) * f32(1.0 / (PQ_M2 * _LOG2E))
    h = f32(1.0) + t * f32(1.0 / 6.0)
    for k in (5.0, 4.0, 3.0, 2.0):
        h = f32(1.0) + (t * f32(1.0 / k)) * h
    u = -(t * h)
    num, den = f32(1.0 - PQ_C1) - u, f32(1.0 - PQ_C1) + f32(PQ_C3) * u
    return np.where(e > 0, _pw(np.where(num > 0, num, f32(0.0)) * _rcp(den), 1.0 / PQ_M1), f32(0.0)).astype(f32)


def _hlg_inv32(e):
    hi = (np.exp2((e - f32(HLG_C)) * f32(_LOG2E / HLG_A)) + f32(HLG_B)) * f32(1.0 / 12.0)
    return np.where(e <= f32(0.5), e * e * f32(1.0 / 3.0), hi).astype(f32)


def _pq_inv32(x):
    p = _pw(x, PQ_M1)
    n, d = f32(1.0 - PQ_C1) * (f32(1.0) - p), f32(1.0) + f32(PQ_C3) * p
    s = n * _rcp((d + d) - n)
    z = s * s
    poly = f32(1.0) + z * (f32(1.0 / 3.0) + z * (f32(0.2) + z * (f32(1.0 / 7.0) + z * f32(1.0 / 9.0))))
    return np.exp2(f32(-2.0 * PQ_M2 * _LOG2E) * (s * poly)).astype(f32)


def itp32(side, H, W, sdr_white=203.0):
    """(I*, T*, P*) = 720 (I, T, P) of a side as the kernel forms them, float32 (N, H, W) each."""
    s0, s1, s2 = samples(side, H, W)
    if side[0] == "sdr":
        lut, k, N = E.decode_table().astype(f32), f32(sdr_white / 10000.0), to_2020().astype(f32)
        lr, lg, lb = k * lut[s0], k * lut[s1], k * lut[s2]
        dr, db = lr - lg, lb - lg
        r, g, b = ((lg + N[i, 0] * dr) + N[i, 2] * db for i in range(3))
    else:
        full = side[4] == "full"
        yo, ys, cs = (0, f32(1.0 / 1023.0), f32(1.0 / 1023.0)) if full else (64, f32(1.0 / 876.0), f32(1.0 / 896.0))
        rv, bu = f32(2.0 * (1.0 - KR)), f32(2.0 * (1.0 - KB))
        gu, gv = f32(-2.0 * KB * (1.0 - KB) / KG), f32(-2.0 * KR * (1.0 - KR) / KG)
        y, cb, cr = (s0 - yo).astype(f32) * ys, (s1 - 512).astype(f32) * cs, (s2 - 512).astype(f32) * cs
        er, eg, eb = (np.clip(v, f32(0.0), f32(1.0)) for v in (y + rv * cr, y + (gu * cb + gv * cr), y + bu * cb))
        if side[3] == "pq":
            r, g, b = _pq_eotf32(er), _pq_eotf32(eg), _pq_eotf32(eb)
        else:
            sr, sg, sb = _hlg_inv32(er), _hlg_inv32(eg), _hlg_inv32(eb)
            f = f32(0.1) * _pw((f32(0.2627) * sr + f32(0.6780) * sg) + f32(0.0593) * sb, 0.2)
            r, g, b = f * sr, f * sg, f * sb
    dr, db = r - g, b - g
    lp, mp, sp = (_pq_inv32((g + f32(c0 / 4096.0) * dr) + f32(c2 / 4096.0) * db) for c0, c2 in ((1688.0, 262.0), (683.0, 462.0), (99.0, 3688.0)))
    lm, sm = lp - mp, sp - mp
    out = (f32(360.0) * (lp + mp), f32(360.0 * 6610.0 / 4096.0) * lm + f32(360.0 * 7003.0 / 4096.0) * sm,
           f32(720.0 * 17933.0 / 4096.0) * lm + f32(-720.0 * 543.0 / 4096.0) * sm)
    assert all(v.dtype == f32 for v in out)
    return out


def delta32(a, b, H, W, sdr_white=203.0):
    """dE_ITP as the kernel forms it (the equal-samples rule included, which changes nothing: both sides run the same operations)."""
    ia, ta, pa = itp32(a, H, W, sdr_white)
    ib, tb, pb = itp32(b, H, W, sdr_white)
    di, dt, dp = ia - ib, ta - tb, pa - pb
    return np.where((dt == 0) & (dp == 0), np.abs(di), np.sqrt((di * di + dt * dt) + dp * dp)).astype(f32)


# ------------------------------------------------------------------------------------------------ frames
KINDS = ("noise", "dark", "near", "ramp", "saturated")


def hdr_pair(fmt, H, W, seed):
    """Two stacks of five payloads, (5, frame bytes) each, in the order of KINDS: noise against other noise (every 10-bit code, so
    codes outside the legal range too); dark against dark (codes just above black, where PQ is steepest); noise against a near copy
    (a share of the samples moved by one code); a ramp against the ramp one code up; extremes against extremes (0 and 1023 on every
    plane: the clamp)."""
    rng = np.random.default_rng(seed)
    ch, cw = R.plane_shapes(fmt, H, W)

    def planes(lo, hi, clo=0, chi=1024):
        return [rng.integers(lo, hi, (1, H, W)), rng.integers(clo, chi, (1, ch, cw)), rng.integers(clo, chi, (1, ch, cw))]

    noise_a, noise_b, dark_a, dark_b, base = planes(0, 1024), planes(0, 1024), planes(60, 90, 500, 525), planes(60, 90, 500, 525), planes(0, 1024)
    near = [np.clip(p + rng.integers(-1, 2, p.shape) * (rng.random(p.shape) < 0.2), 0, 1023) for p in base]
    i = np.arange(H * W).reshape(1, H, W)
    ramp_a = [(i * 7) % 1024, (np.arange(ch * cw).reshape(1, ch, cw) * 5) % 1024, (np.arange(ch * cw).reshape(1, ch, cw) * 11 + 300) % 1024]
    ramp_b = [(ramp_a[0] + 1) % 1024, ramp_a[1], (ramp_a[2] + 1) % 1024]
    sat_a, sat_b = ([rng.integers(0, 2, p.shape) * 1023 for p in base] for _ in range(2))
    a = np.concatenate([R.join_planes(*p, fmt) for p in (noise_a, dark_a, base, ramp_a, sat_a)])
    b = np.concatenate([R.join_planes(*p, fmt) for p in (noise_b, dark_b, near, ramp_b, sat_b)])
    for x in (a, b):
        x.setflags(write=False)
    return a, b


def sdr_pair(H, W, seed):
    """Two stacks of five uint8 frames, (5, H, W, 3), in the order of KINDS."""
    rng = np.random.default_rng(seed)
    noise_a, noise_b, base = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(3))
    dark_a, dark_b = (rng.integers(0, 6, (H, W, 3), dtype=np.uint8) for _ in range(2))
    near = np.clip(base.astype(np.int16) + rng.integers(-1, 2, base.shape) * (rng.random(base.shape) < 0.2), 0, 255).astype(np.uint8)
    i = np.arange(H * W)
    ramp_a = np.stack([i % 256, (i * 3) % 256, (i // 7) % 256], -1).reshape(H, W, 3).astype(np.uint8)
    ramp_b = ((ramp_a.astype(np.int16) + 1) % 256).astype(np.uint8)
    sat_a, sat_b = ((rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8) for _ in range(2))
    a, b = np.stack([noise_a, dark_a, base, ramp_a, sat_a]), np.stack([noise_b, dark_b, near, ramp_b, sat_b])
    for x in (a, b):
        x.setflags(write=False)
    return a, b


# ------------------------------------------------------------------------------------------------ the cases of the tests
# (H, W, side A, side B); a side is "sdr" or (format, transfer, range).  All four formats, both transfers, both ranges and the three
# mixes of kinds, spread over the sizes: 1 x 1 and 2 x 2 (less than a chroma block, one block), 7 x 13 (odd both ways: partial
# chroma blocks), 16 x 32 (16-byte runs), 70 x 530 (ten workgroups, the last one partial).
CASES = [
    (1, 1, ("yuv444p10le", "pq", "limited"), ("yuv444p10le", "pq", "limited")),
    (1, 1, "sdr", "sdr"),
    (2, 2, ("yuv420p10le", "hlg", "full"), ("p010le", "pq", "limited")),
    (2, 2, "sdr", ("yuv422p10le", "pq", "full")),
    (7, 13, ("yuv420p10le", "pq", "limited"), ("yuv420p10le", "pq", "limited")),
    (7, 13, ("yuv422p10le", "hlg", "limited"), "sdr"),
    (7, 13, ("p010le", "hlg", "full"), ("yuv444p10le", "hlg", "limited")),
    (16, 32, ("p010le", "pq", "limited"), ("p010le", "pq", "limited")),
    (16, 32, ("yuv420p10le", "hlg", "limited"), "sdr"),
    (16, 32, "sdr", "sdr"),
    (70, 530, ("yuv420p10le", "pq", "full"), ("yuv422p10le", "hlg", "full")),
    (70, 530, ("yuv444p10le", "pq", "limited"), "sdr"),
    (70, 530, ("p010le", "hlg", "limited"), ("p010le", "pq", "full")),
    (70, 530, "sdr", "sdr"),
]
_cases = {}


def case_id(case):
    H, W, a, b = case
    return f"{H}x{W}-" + "-vs-".join(s if s == "sdr" else "_".join(s) for s in (a, b))


def case_sides(case):
    """The two sides of a case (five frames each, KINDS), the float64 definition and the float32 restatement of their dE_ITP;
    computed once, read-only."""
    if case not in _cases:
        H, W, a, b = case
        seed = 1000 * H + W
        if a == b:
            xa, xb = sdr_pair(H, W, seed) if a == "sdr" else hdr_pair(a[0], H, W, seed)
        else:
            xa = sdr_pair(H, W, seed)[0] if a == "sdr" else hdr_pair(a[0], H, W, seed)[0]
            xb = sdr_pair(H, W, seed + 1)[1] if b == "sdr" else hdr_pair(b[0], H, W, seed + 1)[1]
        sa = sdr(xa) if a == "sdr" else hdr(xa, *a)
        sb = sdr(xb) if b == "sdr" else hdr(xb, *b)
        want, f32v = delta(sa, sb, H, W), delta32(sa, sb, H, W)
        want.setflags(write=False), f32v.setflags(write=False)
        _cases[case] = (sa, sb, want, f32v)
    return _cases[case]


def restatement_deviation():
    """The largest |float32 restatement - definition| over the frames of CASES."""
    return max(float(np.abs(case_sides(c)[3].astype(np.float64) - case_sides(c)[2]).max()) for c in CASES)
