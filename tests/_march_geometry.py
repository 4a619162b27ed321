"""Host-side restatement of the marching-strip kernel's launch geometry (csrc/dichromat_march.hip: MarchCfg and, in
launch_march, set_strips / set_chunks / sw_narrow), plus what the dichromat GPU tests share: seeded frames, one oracle run
per (spec, frame) and the byte comparison that prints where two frames differ.

The restatement only PICKS frame sizes and says what a pin should give; every GPU test checks it against
DichromatOp.last_launch() and never trusts it alone.  tests/test_dichromat_geometry_host.py pins it to hand-computed values."""
import os

import numpy as np

SY = 4  # rows per iteration of every marching instantiation
SEED_1080P, SEED_4K = 11, 12  # the 1080 x 1920 and 2160 x 3840 frames both dichromat GPU files use (one oracle run per species)


def march_cfg(R: int, f64: bool, NG: int):
    """(XPT, SW, SW_CAP, SPEC) of the instantiation march_dispatch picks for (radius, element type, workgroup width)."""
    xpt = 2 if f64 or R not in (1, 3) else 4          # AVX_MARCH_F32(RR, XX, ...): 4 columns per thread for R = 1, 3
    sw = xpt * NG
    spec = NG == 64
    cap = min(64 // (SY // 2) * 4 - 2 * R, sw) if (spec and f64) else sw  # kCapStrips: the cat's producer decodes in one pass
    return xpt, sw, cap, spec


def narrowed_width(R: int, f64: bool, NG: int) -> int:
    """launch_march's sw_narrow: float32 SPEC only; strips that fit one 64-item producer pass less, a multiple of 16 px; 0 = none."""
    xpt, sw, _, spec = march_cfg(R, f64, NG)
    if not spec or f64:
        return 0
    passes = ((SY // 2) * ((sw + 2 * R + 3) // 4) + 63) // 64
    n = (((passes - 1) * 64 // (SY // 2)) * 4 - 2 * R) // 16 * 16 if passes > 1 else 0
    return n if 32 <= n < sw else 0


def set_strips(W: int, cap: int, xpt: int):
    """-> (nstrips, sw): launch_march's set_strips."""
    nstrips = (W + cap - 1) // cap
    sw = ((W + nstrips - 1) // nstrips + xpt - 1) // xpt * xpt
    sw16 = (sw + 15) // 16 * 16
    if sw16 <= cap:
        sw, nstrips = sw16, (W + sw16 - 1) // sw16
    return nstrips, sw


def set_chunks(H: int, nc: int):
    """-> (nchunks, ch): launch_march's set_chunks (the request is clamped to H // 32 chunks, never fewer than 1)."""
    nc = max(1, min(nc, max(1, H // (8 * SY))))
    ch = ((H + nc - 1) // nc + SY - 1) // SY * SY
    return (H + ch - 1) // ch, ch


def expected_launch(R: int, f64: bool, NG: int, n: int, H: int, W: int, chunks: int, narrow: bool = False) -> dict:
    """What last_launch() must report for a pinned marching launch."""
    xpt, _, cap, spec = march_cfg(R, f64, NG)
    if narrow:
        cap = narrowed_width(R, f64, NG)
        assert 0 < cap < W, "the host code narrows strips only for float32 SPEC and frames wider than the narrowed strip"
    nstrips, sw = set_strips(W, cap, xpt)
    nchunks, ch = set_chunks(H, chunks)
    return dict(family="march", R=R, f64=int(f64), NG=NG, spec=int(spec), sw=sw, nstrips=nstrips, ch=ch, nchunks=nchunks,
                xcd_remap=int((n * nstrips * nchunks) % 8 == 0), narrow=int(narrow), grid=n * nstrips * nchunks)


def last_strip_px(W: int, nstrips: int, sw: int) -> int:
    return W - (nstrips - 1) * sw


def last_chunk_rows(H: int, nchunks: int, ch: int) -> int:
    return H - (nchunks - 1) * ch


# ---- shared by the GPU tests ------------------------------------------------------------------------------------------

def frame(seed: int, H: int, W: int, n: int = 0) -> np.ndarray:
    """Seeded random uint8 frame (H, W, 3), or batch (n, H, W, 3)."""
    shape = (n, H, W, 3) if n else (H, W, 3)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


_ORACLE = {}


def oracle_bytes(oracle, spec_key: str, spec, frame_key, image: np.ndarray) -> np.ndarray:
    """oracle.dichromat_visualize(spec, image)[1], computed once per (spec_key, frame_key) and kept for the session."""
    key = (spec_key, frame_key)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.dichromat_visualize(spec, image)[1]
        assert _ORACLE[key].dtype == np.uint8 and _ORACLE[key].shape == image.shape
    return _ORACLE[key]


def assert_same_bytes(got: np.ndarray, want: np.ndarray, what: str, launch=None):
    """np.array_equal, and on failure: how many bytes differ, their bounding box, and the launch that produced them."""
    if np.array_equal(got, want):
        return
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    idx = np.nonzero((got != want).reshape(-1, *got.shape[-3:]).any(axis=-1))
    box = ", ".join(f"{nm} {int(i.min())}..{int(i.max())}" for nm, i in zip(("frame", "row", "col"), idx))
    raise AssertionError(f"{what}: {int((got != want).sum())} bytes differ from the oracle ({box}); launch: {launch}")


def unset_march_pins(monkeypatch):
    for k in ("AVX_MARCH_NG", "AVX_MARCH_CHUNKS", "AVX_MARCH_SWCAP", "AVX_MARCH_NOSEED", "AVX_VARIANT", "AVX_ABLATE", "AVX_STAMPS"):
        monkeypatch.delenv(k, raising=False)
    assert not any(k.startswith("AVX_MARCH_") for k in os.environ)
