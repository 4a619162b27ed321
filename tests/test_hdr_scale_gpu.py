"""GPU: the scaled HDR decode (csrc/yuv_hdr_scale.hip) bit for bit against the chain it replaces -- yuv.yuv_hdr_to_rgb,
then geometry.resize(..., INTER_AREA) per frame, both run here on the same device -- for the four 10-bit formats and both transfers
on the integer-ratio, the 2 x 2 vector and the general-ratio kernels; an anchor on the float64 definition that runs none of the
code under test; the C entry point's argument checks; FramePipeline(transfer=, scale=), VideoRenderer and the `video` command on
top of it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _hdr_ref as H
import _rawyuv_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

FMTS_420 = ["yuv420p10le", "p010le"]
# (H, W) -> (Hd, Wd): 2x2 (the (sum + 2) >> 2 case); 3x4 (rint, mixed ratios); 3x3 on odd sizes (chroma blocks straddle destination
# pixels, odd last row and column); 1x2 (one axis kept); the smallest frame; the identity
INT_CASES = [((96, 160), (48, 80)), ((96, 160), (32, 40)), ((99, 165), (33, 55)), ((96, 162), (96, 81)), ((2, 2), (1, 1)), ((97, 161), (97, 161))]
# both axes non-integer; one axis an integer ratio and the other not; 1.5x
GEN_CASES = [((97, 161), (64, 100)), ((97, 161), (97, 80)), ((108, 192), (72, 128))]


def _settings(fmt, transfer, k):
    """The (range, tone map) pairs of _hdr_ref.COMBOS for `transfer`, rotated over the cases and the formats."""
    pairs = [(r, m) for t, r, m in H.COMBOS if t == transfer]
    return pairs[(k + H.FORMATS.index(fmt)) % len(pairs)]


def _resize(rgb, Hd, Wd):
    from animal_vision_amd.geometry import INTER_AREA, resize

    return resize(np.ascontiguousarray(rgb), (Wd, Hd), INTER_AREA)


def _chain(buf, fmt, Hh, W, Hd, Wd, transfer, **kw):
    """The definition: the HDR decode of each frame, then the uint8 INTER_AREA resize of that frame."""
    from animal_vision_amd.yuv import yuv_hdr_to_rgb

    buf = np.asarray(buf)
    frames = buf if buf.ndim == 2 else buf[None]
    out = np.stack([_resize(yuv_hdr_to_rgb(f, Hh, W, pix_fmt=fmt, transfer=transfer, **kw), Hd, Wd) for f in frames])
    return out if buf.ndim == 2 else out[0]


def _check_cases(fmt, transfer, cases):
    from animal_vision_amd.yuv import yuv_hdr_to_rgb_scaled

    for k, ((Hh, W), (Hd, Wd)) in enumerate(cases):
        rng, tm = _settings(fmt, transfer, k)
        kw = dict(range=rng, tonemap=tm)
        buf = R.random_payload(fmt, 3, Hh, W, seed=Hh * 7 + W + Hd)
        got = yuv_hdr_to_rgb_scaled(buf, Hh, W, Hd, Wd, pix_fmt=fmt, transfer=transfer, **kw)
        assert got.shape == (3, Hd, Wd, 3) and got.dtype == np.uint8
        assert np.array_equal(got, _chain(buf, fmt, Hh, W, Hd, Wd, transfer, **kw)), (fmt, transfer, Hh, W, Hd, Wd, rng, tm)
        for j in range(3):
            one = yuv_hdr_to_rgb_scaled(buf[j], Hh, W, Hd, Wd, pix_fmt=fmt, transfer=transfer, **kw)
            assert np.array_equal(one, got[j]), (fmt, transfer, Hh, W, Hd, Wd, j)


# ---------------------------------------------------------------- kernels ------------------------------------------------------
@pytest.mark.parametrize("transfer", H.TRANSFERS)
@pytest.mark.parametrize("fmt", H.FORMATS)
def test_integer_ratios_equal_the_chain_and_batch_equals_frame_by_frame(fmt, transfer):
    _check_cases(fmt, transfer, INT_CASES)


@pytest.mark.parametrize("transfer", H.TRANSFERS)
@pytest.mark.parametrize("fmt", H.FORMATS)
def test_identity_equals_the_hdr_decode(fmt, transfer):
    from animal_vision_amd.yuv import yuv_hdr_to_rgb, yuv_hdr_to_rgb_scaled

    Hh, W = 97, 161
    buf = R.random_payload(fmt, 2, Hh, W, seed=5)
    assert np.array_equal(yuv_hdr_to_rgb_scaled(buf, Hh, W, Hh, W, pix_fmt=fmt, transfer=transfer),
                          yuv_hdr_to_rgb(buf, Hh, W, pix_fmt=fmt, transfer=transfer))


@pytest.mark.parametrize("transfer", H.TRANSFERS)
@pytest.mark.parametrize("fmt", H.FORMATS)
def test_general_ratios_equal_the_chain_and_batch_equals_frame_by_frame(fmt, transfer):
    _check_cases(fmt, transfer, GEN_CASES)


def _scaled_at_offsets(ctx, buf, fmt, Hh, W, Hd, Wd, transfer, src_off, dst_off):
    """The entry point on one frame whose payload sits src_off bytes and whose destination sits dst_off bytes into 256-byte aligned
    allocations."""
    from animal_vision_amd._lib import AVX_PIX_FMTS, AVX_TRANSFERS, lib

    d_in, d_out = ctx.malloc(buf.nbytes + 64), ctx.malloc(Hd * Wd * 3 + 64)
    try:
        assert d_in.ptr % 16 == 0 and d_out.ptr % 16 == 0
        ctx.upload(buf, d_in.view(src_off, buf.nbytes))
        dst = d_out.view(dst_off, Hd * Wd * 3)
        ctx._check(lib.avx_yuv_hdr_to_rgb_scaled_u8(ctx._h, AVX_PIX_FMTS[fmt], d_in.ptr + src_off, dst.ptr, 1, Hh, W, Hd, Wd, 0, AVX_TRANSFERS[transfer],
                                                    1, 1000.0, 203.0, ctx.stream))
        return ctx.download(dst, (Hd, Wd, 3), np.uint8)
    finally:
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("transfer", H.TRANSFERS)
@pytest.mark.parametrize("fmt", FMTS_420)
@pytest.mark.parametrize("Hh,W", [(2, 32), (64, 128), (32, 48)])
def test_vector_path_equals_the_chain_and_the_per_pixel_path(fmt, transfer, Hh, W):
    """W % 32 == 0 and H even with 16-byte aligned buffers: the 2 x 2 vector kernel (one unit; several units per row); (32, 48) has
    W % 16 == 0 only and stays on the per-pixel kernel.  The same frame from a payload, then into a destination, 8 bytes off
    alignment takes the per-pixel kernel: the bytes must be equal."""
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    Hd, Wd = Hh // 2, W // 2
    buf = R.random_payload(fmt, 1, Hh, W, seed=Hh + len(fmt))[0]
    want = _chain(buf, fmt, Hh, W, Hd, Wd, transfer)
    assert np.array_equal(_scaled_at_offsets(ctx, buf, fmt, Hh, W, Hd, Wd, transfer, 0, 0), want)
    assert np.array_equal(_scaled_at_offsets(ctx, buf, fmt, Hh, W, Hd, Wd, transfer, 8, 0), want)
    assert np.array_equal(_scaled_at_offsets(ctx, buf, fmt, Hh, W, Hd, Wd, transfer, 0, 8), want)


@pytest.mark.parametrize("transfer", H.TRANSFERS)
def test_vector_path_batch_of_three(transfer):
    from animal_vision_amd.yuv import yuv_hdr_to_rgb_scaled

    Hh, W = 64, 128
    for fmt in FMTS_420:
        buf = R.random_payload(fmt, 3, Hh, W, seed=3)
        assert np.array_equal(yuv_hdr_to_rgb_scaled(buf, Hh, W, 32, 64, pix_fmt=fmt, transfer=transfer),
                              _chain(buf, fmt, Hh, W, 32, 64, transfer)), fmt


def test_one_1080p_p010le_pq_frame_to_540p():
    from animal_vision_amd.yuv import yuv_hdr_to_rgb_scaled

    Hh, W = 1080, 1920
    buf = R.random_payload("p010le", 1, Hh, W, seed=1080)[0]
    got = yuv_hdr_to_rgb_scaled(buf, Hh, W, 540, 960, pix_fmt="p010le", transfer="pq")
    assert np.array_equal(got, _chain(buf, "p010le", Hh, W, 540, 960, "pq"))


@pytest.mark.parametrize("dst", [(48, 80), (64, 100)])
def test_p010le_equals_yuv420p10le_on_the_same_samples(dst):
    from animal_vision_amd.yuv import yuv_hdr_to_rgb_scaled

    Hh, W = 96, 160
    p010 = R.random_payload("p010le", 2, Hh, W, seed=Hh)  # random low 6 bits: ignored on read
    assert (p010[:, 0::2] & 63).any()
    planar = R.join_planes(*R.split_planes(p010, "p010le", Hh, W), "yuv420p10le")
    for transfer in H.TRANSFERS:
        assert np.array_equal(yuv_hdr_to_rgb_scaled(p010, Hh, W, *dst, pix_fmt="p010le", transfer=transfer),
                              yuv_hdr_to_rgb_scaled(planar, Hh, W, *dst, pix_fmt="yuv420p10le", transfer=transfer)), (dst, transfer)


# ---------------------------------------------------------------- an anchor that runs none of the code under test -------------------
def _block_mean(rgb, bh, bw):
    """NumPy's INTER_AREA of an integer ratio on uint8 codes: (sum + 2) >> 2 for 2 x 2, else rint(sum / area)."""
    n, Hh, W, _ = rgb.shape
    s = rgb.astype(np.int64).reshape(n, Hh // bh, bh, W // bw, bw, 3).sum((2, 4))
    return (s + 2) >> 2 if (bh, bw) == (2, 2) else np.rint(s / float(bh * bw)).astype(np.int64)


@pytest.mark.parametrize("transfer", H.TRANSFERS)
@pytest.mark.parametrize("dst", [(48, 80), (32, 40)])
def test_within_one_code_of_the_block_mean_of_the_definition(dst, transfer):
    """Every decoded sample is within one code of the float64 definition, and the block mean and its rounding are
    monotone in every sample: the reduced frame is within one code of the block mean of the definition's frame."""
    from animal_vision_amd.yuv import yuv_hdr_to_rgb_scaled

    Hh, W = 96, 160
    Hd, Wd = dst
    for k, fmt in enumerate(H.FORMATS):
        rng, tm = _settings(fmt, transfer, k)
        buf = R.random_payload(fmt, 2, Hh, W, seed=17 + k)
        got = yuv_hdr_to_rgb_scaled(buf, Hh, W, Hd, Wd, pix_fmt=fmt, transfer=transfer, range=rng, tonemap=tm)
        want = _block_mean(H.decode(buf, fmt, Hh, W, transfer, rng, tm), Hh // Hd, W // Wd)
        assert int(np.abs(got.astype(np.int64) - want).max()) <= 1, (fmt, transfer, dst, rng, tm)


@pytest.mark.parametrize("transfer", H.TRANSFERS)
def test_neutral_payloads_stay_neutral_and_limited_black_is_black(transfer):
    from animal_vision_amd.yuv import yuv_hdr_to_rgb_scaled

    Hh, W = 96, 160
    g = np.random.default_rng(6)
    for fmt in H.FORMATS:
        ch, cw = R.plane_shapes(fmt, Hh, W)
        C = np.full((1, ch, cw), 512)
        Y = g.integers(0, 1024, (1, Hh, W))
        for dst in ((48, 80), (32, 40), (64, 100)):
            got = yuv_hdr_to_rgb_scaled(R.join_planes(Y, C, C, fmt)[0], Hh, W, *dst, pix_fmt=fmt, transfer=transfer)
            assert (got[..., 0] == got[..., 1]).all() and (got[..., 1] == got[..., 2]).all(), (fmt, dst)
            black = yuv_hdr_to_rgb_scaled(R.join_planes(np.full((1, Hh, W), 64), C, C, fmt)[0], Hh, W, *dst, pix_fmt=fmt, transfer=transfer)
            assert not black.any(), (fmt, dst)


# ---------------------------------------------------------------- the entry point's argument checks --------------------------------
def test_bad_arguments_return_invalid_with_the_name_first():
    from animal_vision_amd._lib import AVX_ERR_INVALID, AVX_OK, lib
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    d = ctx.malloc(8192)
    a, b = d.ptr, d.ptr + 4096
    inf, nan = float("inf"), float("nan")
    names = ("fmt", "yuv", "rgb", "n", "H", "W", "Hd", "Wd", "full_range", "transfer", "tonemap", "peak_nits", "sdr_white")
    ok = (8, a, b, 1, 8, 8, 4, 4, 0, 1, 1, 1000.0, 203.0)
    fn = lib.avx_yuv_hdr_to_rgb_scaled_u8

    def but(**kw):
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    try:
        assert fn(ctx._h, *ok, ctx.stream) == AVX_OK
        ctx.sync()
        bad = [but(fmt=0), but(fmt=1), but(fmt=2), but(fmt=3), but(fmt=4), but(fmt=9), but(fmt=-1),  # 8-bit formats, gray, no format
               but(transfer=0), but(transfer=3), but(tonemap=-1), but(tonemap=2),
               but(peak_nits=203.0), but(peak_nits=100.0), but(peak_nits=inf), but(peak_nits=nan), but(sdr_white=0.0), but(sdr_white=-203.0),
               but(sdr_white=nan), but(sdr_white=inf), but(peak_nits=-5.0, sdr_white=-10.0),
               but(n=0), but(H=0), but(W=-8), but(H=1 << 16), but(Hd=0), but(Wd=-4), but(full_range=2),
               but(Hd=9), but(Wd=9),                                                                 # enlarging on either axis
               but(yuv=0), but(rgb=0), but(rgb=a), but(rgb=a + 64), but(yuv=a + 16, rgb=a),          # NULL, overlapping
               but(yuv=a + 1), but(fmt=5, yuv=a + 1)]                                                # an odd payload address
        for args in bad:
            assert fn(ctx._h, *args, ctx.stream) == AVX_ERR_INVALID, args
            assert lib.avx_last_error(ctx._h).decode().startswith("avx_yuv_hdr_to_rgb_scaled_u8"), args
        assert fn(None, *ok, ctx.stream) == AVX_ERR_INVALID
    finally:
        d.free()


def test_a_256_x_256_block_is_accepted_and_a_512_x_256_block_is_refused():
    """65536 samples per output pixel is the last size the integer argument covers: 255 * 65536 < 2^24."""
    from animal_vision_amd._lib import AVX_ERR_INVALID, lib
    from animal_vision_amd.runtime import get_context
    from animal_vision_amd.yuv import yuv_hdr_to_rgb_scaled

    fmt = "yuv444p10le"
    buf = R.random_payload(fmt, 1, 256, 256, seed=1)[0]
    assert np.array_equal(yuv_hdr_to_rgb_scaled(buf, 256, 256, 1, 1, pix_fmt=fmt, transfer="pq"), _chain(buf, fmt, 256, 256, 1, 1, "pq"))
    ctx = get_context()
    d = ctx.malloc(R.frame_size(fmt, 512, 256) + 4096)
    try:
        far = d.ptr + R.frame_size(fmt, 512, 256) + 1024  # past the payload
        assert lib.avx_yuv_hdr_to_rgb_scaled_u8(ctx._h, 7, d.ptr, far, 1, 512, 256, 1, 1, 0, 1, 1, 1000.0, 203.0, ctx.stream) == AVX_ERR_INVALID
        msg = lib.avx_last_error(ctx._h).decode()
        assert msg.startswith("avx_yuv_hdr_to_rgb_scaled_u8") and "65536" in msg
    finally:
        d.free()


# ---------------------------------------------------------------- FramePipeline(transfer=, scale=) ----------------------------------
def _run(pipe, frames):
    got = {}
    pipe.run(((i, f) for i, f in enumerate(frames)), lambda i, o: got.__setitem__(i, o))
    pipe.close()
    return [got[i] for i in range(len(frames))]


def _dog():
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp

    return DichromatOp(Dog.SPEC)


@pytest.mark.parametrize("fmt,transfer,src,dst", [("p010le", "pq", (96, 160), (48, 80)), ("yuv422p10le", "hlg", (97, 161), (64, 100))])
def test_scaled_hdr_pipeline_equals_the_composition_by_hand_and_keeps_no_source_size_buffer(fmt, transfer, src, dst):
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.yuv import rgb_to_yuv

    (Hh, W), (Hd, Wd) = src, dst
    yuv = R.random_payload(fmt, 6, Hh, W, seed=W + Hd)
    small = list(_chain(yuv, fmt, Hh, W, Hd, Wd, transfer))
    hdr = dict(io_format="yuv", pix_fmt=fmt, transfer=transfer, scale=(Wd, Hd))
    for split in (False, True):
        want = _run(FramePipeline(_dog(), Hd, Wd, depth=3, split_compare=split), small)
        outs = []
        for batch in (1, 4):
            pipe = FramePipeline(_dog(), Hh, W, depth=3, split_compare=split, batch=batch, **hdr)
            assert (pipe.H, pipe.W, pipe.out_H, pipe.out_W) == (Hh, W, Hd, Wd) and pipe.out_matrix == "bt709"
            assert all(s.d_full is None for s in pipe.slots)
            outs.append(_run(pipe, list(yuv)))
        for k in range(len(yuv)):
            assert outs[0][k].shape == (R.frame_size(fmt, Hd, Wd),)  # --split-compare too has the scaled size
            assert np.array_equal(outs[0][k], rgb_to_yuv(want[k], pix_fmt=fmt, matrix="bt709")), (split, k)
            assert np.array_equal(outs[1][k], outs[0][k]), (split, k)  # batch 4 equals batch 1
    pipe = FramePipeline(_dog(), Hh, W, scale=(Wd, Hd))  # io_format="rgb" still reduces out of a source-size buffer
    assert all(s.d_full is not None and s.d_full.nbytes == Hh * W * 3 for s in pipe.slots)
    pipe.close()


# ---------------------------------------------------------------- VideoRenderer and the command -------------------------------------
def test_get_image_of_an_hdr_source_with_a_scale_equals_the_chain(tmp_path):
    from animal_vision_amd.renderers import VideoRenderer

    Hh, W, Hd, Wd, fmt = 97, 161, 64, 100, "p010le"
    yuv = R.random_payload(fmt, 2, Hh, W, seed=6)
    src = str(tmp_path / "in.yuv")
    with open(src, "wb") as f:
        f.write(yuv.tobytes())
    vr = VideoRenderer(read_path=src, pix_fmt=fmt, size=(W, Hh), transfer="hlg", tonemap="clip", scale=(Wd, Hd))
    vr.open()
    want = _chain(yuv, fmt, Hh, W, Hd, Wd, "hlg", tonemap="clip")
    for k in range(2):
        assert np.array_equal(vr.get_image(), want[k]), k
    assert vr.get_image() is None
    vr.close()


def test_cli_p010le_hlg_scaled_through_a_child_process_equals_the_pipeline(tmp_path):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.pipeline import FramePipeline

    Hh, W, Hd, Wd, fmt = 64, 96, 32, 48, "p010le"
    yuv = R.random_payload(fmt, 4, Hh, W, seed=9)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "dog.yuv")
    with open(src, "wb") as f:
        f.write(yuv.tobytes())
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "animal_vision_amd.video", src, dst, "--species", "Dog", "--pix-fmt", fmt, "--size", f"{W}x{Hh}",
                          "--transfer", "hlg", "--scale", f"{Wd}x{Hd}"], capture_output=True, timeout=180, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    assert b"4 frames" in out.stderr
    raw = open(dst, "rb").read()
    assert len(raw) == 4 * R.frame_size(fmt, Hd, Wd)
    want = _run(FramePipeline(Dog()._operator(), Hh, W, io_format="yuv", pix_fmt=fmt, transfer="hlg", scale=(Wd, Hd)), list(yuv))
    assert raw == b"".join(w.tobytes() for w in want)
