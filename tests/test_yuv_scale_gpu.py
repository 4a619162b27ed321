"""GPU: the scaled decode (csrc/yuv_scale.hip) bit for bit against the chain it replaces -- avx_yuv_to_rgb_u8, then
avx_resize_hwc(uint8, INTER_AREA) per frame, both called here -- for every format on the integer-ratio, the 2 x 2 vector and the
general-ratio kernels; FramePipeline(scale=), run_video and the `video` command's --scale on top of it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _rawyuv_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

FMTS = list(R.FORMATS)
FMTS_420 = ["yuv420p", "nv12", "yuv420p10le", "p010le"]
# (H, W) -> (Hd, Wd): 2x2 (the (sum + 2) >> 2 case); 3x4 (rint, mixed ratios); 3x3 on odd sizes (chroma blocks straddle destination
# pixels, odd last row and column); 1x2 (one axis kept); the smallest frame; the identity
INT_CASES = [((96, 160), (48, 80)), ((96, 160), (32, 40)), ((99, 165), (33, 55)), ((96, 162), (96, 81)), ((2, 2), (1, 1)), ((97, 161), (97, 161))]
# general ratios; one axis an integer ratio and the other not; 1.5x (1080p -> 720p)
GEN_CASES = [((97, 161), (64, 100)), ((97, 161), (97, 80)), ((108, 192), (72, 128))]


def _frames(n, H, W, seed=0):
    from animal_vision_amd.synthetic import structured_frame

    return np.stack([structured_frame(seed + k, H, W) for k in range(n)])


def _resize(rgb, Hd, Wd):
    from animal_vision_amd.geometry import INTER_AREA, resize

    return resize(np.ascontiguousarray(rgb), (Wd, Hd), INTER_AREA)


def _chain(buf, fmt, H, W, Hd, Wd, matrix="bt601", rng="limited"):
    """The definition: the plain decode of each frame, then the uint8 INTER_AREA resize of that frame."""
    from animal_vision_amd.yuv import yuv_to_rgb

    buf = np.asarray(buf)
    frames = buf if buf.ndim == 2 else buf[None]
    out = np.stack([_resize(yuv_to_rgb(f, H, W, pix_fmt=fmt, matrix=matrix, range=rng), Hd, Wd) for f in frames])
    return out if buf.ndim == 2 else out[0]


def _check_cases(fmt, cases):
    from animal_vision_amd.yuv import yuv_to_rgb_scaled

    for k, ((H, W), (Hd, Wd)) in enumerate(cases):
        matrix, rng = R.COMBOS[k % 4]
        buf = R.random_payload(fmt, 3, H, W, seed=H * 7 + W + Hd)
        got = yuv_to_rgb_scaled(buf, H, W, Hd, Wd, pix_fmt=fmt, matrix=matrix, range=rng)
        assert got.shape == (3, Hd, Wd, 3) and got.dtype == np.uint8
        assert np.array_equal(got, _chain(buf, fmt, H, W, Hd, Wd, matrix, rng)), (fmt, H, W, Hd, Wd, matrix, rng)
        for j in range(3):
            assert np.array_equal(yuv_to_rgb_scaled(buf[j], H, W, Hd, Wd, pix_fmt=fmt, matrix=matrix, range=rng), got[j]), (fmt, H, W, Hd, Wd, j)


# ---------------------------------------------------------------- kernels ------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_integer_ratios_equal_the_chain_and_batch_equals_frame_by_frame(fmt):
    _check_cases(fmt, INT_CASES)


@pytest.mark.parametrize("fmt", FMTS)
def test_identity_equals_the_plain_decode(fmt):
    from animal_vision_amd.yuv import yuv_to_rgb, yuv_to_rgb_scaled

    H, W = 97, 161
    buf = R.random_payload(fmt, 2, H, W, seed=5)
    assert np.array_equal(yuv_to_rgb_scaled(buf, H, W, H, W, pix_fmt=fmt), yuv_to_rgb(buf, H, W, pix_fmt=fmt))


@pytest.mark.parametrize("fmt", FMTS)
def test_general_ratios_equal_the_chain_and_batch_equals_frame_by_frame(fmt):
    _check_cases(fmt, GEN_CASES)


def _blocks_with_sums(sums, bh, bw):
    """A luma plane whose bh x bw block (i, j) sums to sums[i, j]: every sample the quotient, the first `remainder` samples one more."""
    n = bh * bw
    q, r = np.divmod(np.asarray(sums), n)
    assert (q + (r > 0)).max() <= 255
    blk = q[:, :, None] + (np.arange(n)[None, None, :] < r[:, :, None])
    Hd, Wd = q.shape
    return blk.reshape(Hd, Wd, bh, bw).transpose(0, 2, 1, 3).reshape(Hd * bh, Wd * bw)


def test_rounding_is_half_to_even_as_the_chain_rounds():
    """yuv444p, full range, neutral chroma: every channel decodes to the luma sample, so the block sums are chosen freely.
    3 x 3 blocks: a sum over 9 samples never scales to an exact half (9 n + 4.5 is no integer), so they carry the sums nearest a
    half on either side, 9 n + 4 and 9 n + 5, for every n, next to 0 and 9 * 255; the exact halves are pinned with blocks whose
    area is a power of two and so scales exactly: 1 x 2 (odd sums -> n + .5) and 2 x 4 (sums 8 n + 4 -> n + .5), every n.  Half
    to even: n + .5 -> the even one of n, n + 1."""
    from animal_vision_amd.yuv import yuv_to_rgb, yuv_to_rgb_scaled

    def run(Y, Hd, Wd):
        H, W = Y.shape
        c = np.full((1, H, W), 128)
        buf = R.join_planes(Y[None], c, c, "yuv444p")[0]
        assert np.array_equal(yuv_to_rgb(buf, H, W, pix_fmt="yuv444p", range="full")[..., 1], Y)  # decodes to the luma
        got = yuv_to_rgb_scaled(buf, H, W, Hd, Wd, pix_fmt="yuv444p", range="full")
        assert np.array_equal(got, _chain(buf, "yuv444p", H, W, Hd, Wd, "bt601", "full"))
        return got[..., 0].astype(np.int64)

    n = np.arange(255)
    sums = np.concatenate([9 * n + 4, 9 * n + 5, [0, 9 * 255]]).reshape(16, 32)
    got = run(_blocks_with_sums(sums, 3, 3), 16, 32)
    assert np.array_equal(got, np.rint(sums / 9.0).astype(np.int64))
    for bh, bw, area in ((1, 2, 2), (2, 4, 8)):
        sums = np.concatenate([area * n + area // 2, [0]]).reshape(8, 32)
        got = run(_blocks_with_sums(sums, bh, bw), 8, 32)
        half = np.concatenate([n + (n & 1), [0]]).reshape(8, 32)  # n + .5 -> even
        assert np.array_equal(got, half), (bh, bw)


def _scaled_at_offsets(ctx, buf, fmt, H, W, Hd, Wd, src_off, dst_off):
    """The entry point on one frame whose payload sits src_off bytes and whose destination sits dst_off bytes into 256-byte aligned
    allocations."""
    from animal_vision_amd._lib import AVX_PIX_FMTS, lib

    d_in, d_out = ctx.malloc(buf.nbytes + 64), ctx.malloc(Hd * Wd * 3 + 64)
    try:
        assert d_in.ptr % 16 == 0 and d_out.ptr % 16 == 0
        ctx.upload(buf, d_in.view(src_off, buf.nbytes))
        dst = d_out.view(dst_off, Hd * Wd * 3)
        ctx._check(lib.avx_yuv_to_rgb_scaled_u8(ctx._h, AVX_PIX_FMTS[fmt], d_in.ptr + src_off, dst.ptr, 1, H, W, Hd, Wd, 1, 0, ctx.stream))
        return ctx.download(dst, (Hd, Wd, 3), np.uint8)
    finally:
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("fmt", FMTS_420)
@pytest.mark.parametrize("H,W", [(2, 32), (64, 128), (32, 48), (1080, 1920)])
def test_vector_path_equals_the_chain_and_the_block_path(fmt, H, W):
    """W % 32 == 0 and H even with 16-byte aligned buffers: the 2 x 2 vector kernel; (2, 32) is a single unit, one row pair.  The
    same frame from a payload, then from a destination, 8 bytes off alignment takes the one-thread-per-pixel kernel: the bytes must
    be equal.  (32, 48): W % 32 != 0, the per-pixel kernel at every offset."""
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    Hd, Wd = H // 2, W // 2
    buf = R.random_payload(fmt, 1, H, W, seed=H + len(fmt))[0]
    want = _chain(buf, fmt, H, W, Hd, Wd, "bt709", "limited")
    assert np.array_equal(_scaled_at_offsets(ctx, buf, fmt, H, W, Hd, Wd, 0, 0), want)
    assert np.array_equal(_scaled_at_offsets(ctx, buf, fmt, H, W, Hd, Wd, 8, 0), want)
    assert np.array_equal(_scaled_at_offsets(ctx, buf, fmt, H, W, Hd, Wd, 0, 8), want)


def test_vector_path_batch_of_three():
    from animal_vision_amd.yuv import yuv_to_rgb_scaled

    H, W = 64, 128
    for fmt in FMTS_420:
        buf = R.random_payload(fmt, 3, H, W, seed=3)
        assert np.array_equal(yuv_to_rgb_scaled(buf, H, W, 32, 64, pix_fmt=fmt), _chain(buf, fmt, H, W, 32, 64)), fmt


def test_one_p010le_4k_frame_to_1080p():
    from animal_vision_amd.yuv import yuv_to_rgb_scaled

    H, W = 2160, 3840
    buf = R.random_payload("p010le", 1, H, W, seed=2160)[0]
    got = yuv_to_rgb_scaled(buf, H, W, 1080, 1920, pix_fmt="p010le", matrix="bt709")
    assert np.array_equal(got, _chain(buf, "p010le", H, W, 1080, 1920, "bt709", "limited"))


@pytest.mark.parametrize("matrix,rng", R.COMBOS)
def test_both_matrices_and_ranges_at_depth_8_and_10(matrix, rng):
    from animal_vision_amd.yuv import yuv_to_rgb_scaled

    H, W = 96, 160
    for fmt in ("nv12", "yuv422p10le"):
        buf = R.random_payload(fmt, 2, H, W, seed=8)
        for Hd, Wd in ((48, 80), (32, 40), (50, 90)):
            assert np.array_equal(yuv_to_rgb_scaled(buf, H, W, Hd, Wd, pix_fmt=fmt, matrix=matrix, range=rng),
                                  _chain(buf, fmt, H, W, Hd, Wd, matrix, rng)), (fmt, Hd, Wd)


def test_bad_arguments_return_invalid():
    """Argument checks only: every call returns before anything is launched."""
    from animal_vision_amd._lib import AVX_ERR_INVALID, lib
    from animal_vision_amd.runtime import get_context
    from animal_vision_amd.yuv import yuv_to_rgb_scaled

    ctx = get_context()
    d = ctx.malloc(512 * 512 + 8192)
    a, b = d.ptr, d.ptr + 4096
    far = d.ptr + 512 * 512 + 4096  # past a 512 x 512 gray payload at `a`
    fn = lib.avx_yuv_to_rgb_scaled_u8
    try:
        # (fmt, yuv, rgb, n, H, W, Hd, Wd, matrix, full_range)
        bad = [(1, a, b, 1, 8, 8, 9, 8, 0, 0), (1, a, b, 1, 8, 8, 8, 9, 0, 0),  # enlarging on either axis
               (9, a, b, 1, 8, 8, 4, 4, 0, 0), (-1, a, b, 1, 8, 8, 4, 4, 0, 0), (1, a, b, 1, 8, 8, 4, 4, 2, 0), (1, a, b, 1, 8, 8, 4, 4, 0, 2),
               (1, a, b, 0, 8, 8, 4, 4, 0, 0), (1, a, b, 1, 0, 8, 4, 4, 0, 0), (1, a, b, 1, 8, -8, 4, 4, 0, 0), (1, a, b, 1, 8, 8, 0, 4, 0, 0),
               (1, a, b, 1, 8, 8, 4, -4, 0, 0), (1, a, b, 1, 1 << 16, 8, 4, 4, 0, 0),
               (1, 0, b, 1, 8, 8, 4, 4, 0, 0), (1, a, 0, 1, 8, 8, 4, 4, 0, 0), (1, a, a, 1, 8, 8, 4, 4, 0, 0), (1, a, a + 64, 1, 8, 8, 4, 4, 0, 0),
               (1, a + 16, a, 1, 8, 8, 4, 4, 0, 0),
               (8, a + 1, b, 1, 8, 8, 4, 4, 0, 0), (5, a + 1, b, 1, 8, 8, 4, 4, 0, 0)]  # an odd address with 16-bit samples
        for args in bad:
            assert fn(ctx._h, *args, ctx.stream) == AVX_ERR_INVALID, args
            assert lib.avx_last_error(ctx._h).decode().startswith("avx_yuv_to_rgb_scaled_u8"), args
        # an integer-ratio block of more than 65536 samples: 512 x 512 -> 1 x 1
        assert fn(ctx._h, 4, a, far, 1, 512, 512, 1, 1, 0, 0, ctx.stream) == AVX_ERR_INVALID
        msg = lib.avx_last_error(ctx._h).decode()
        assert msg.startswith("avx_yuv_to_rgb_scaled_u8") and "65536" in msg
        assert fn(None, 1, a, b, 1, 8, 8, 4, 4, 0, 0, ctx.stream) == AVX_ERR_INVALID
    finally:
        d.free()
    with pytest.raises(ValueError):
        yuv_to_rgb_scaled(np.zeros(96, np.uint8), 8, 8, 9, 8, pix_fmt="nv12")
    with pytest.raises(ValueError):
        yuv_to_rgb_scaled(np.zeros(96, np.uint8), 8, 8, 0, 4, pix_fmt="nv12")
    with pytest.raises(ValueError):
        yuv_to_rgb_scaled(np.zeros(10, np.uint8), 8, 8, 4, 4, pix_fmt="nv12")
    with pytest.raises(ValueError):
        yuv_to_rgb_scaled(np.zeros(96, np.uint8), 8, 8, 4, 4, pix_fmt="nv21")


def test_a_256_x_256_block_is_accepted():
    """65536 samples per output pixel is the last size the integer argument covers: 255 * 65536 < 2^24."""
    from animal_vision_amd.yuv import yuv_to_rgb_scaled

    buf = R.random_payload("gray", 1, 256, 256, seed=1)[0]
    assert np.array_equal(yuv_to_rgb_scaled(buf, 256, 256, 1, 1, pix_fmt="gray"), _chain(buf, "gray", 256, 256, 1, 1))


# ---------------------------------------------------------------- FramePipeline(scale=) ------------------------------------------
def _run(pipe, frames):
    got = {}
    pipe.run(((i, f) for i, f in enumerate(frames)), lambda i, o: got.__setitem__(i, o))
    pipe.close()
    return [got[i] for i in range(len(frames))]


def _op(species, H, W, batch=1):
    from animal_vision_amd.animals import Dog, Reindeer
    from animal_vision_amd.animals._uv_species import SpeciesStreamOp
    from animal_vision_amd.dichromat import DichromatOp

    if species == "dog":
        return DichromatOp(Dog.SPEC), None
    op = SpeciesStreamOp(Reindeer(), H, W, depth=3, batch=batch)
    return op, op.close


@pytest.mark.parametrize("fmt", ["nv12", "p010le"])
@pytest.mark.parametrize("species", ["dog", "reindeer"])
@pytest.mark.parametrize("src,dst", [((96, 160), (48, 80)), ((97, 161), (64, 100))])
def test_scaled_yuv_pipeline_equals_rgb_pipeline_of_the_chain_through_the_encode(species, src, dst, fmt):
    from animal_vision_amd.pipeline import FramePipeline

    (H, W), (Hd, Wd) = src, dst
    yuv = R.encode(_frames(5, H, W, seed=11), fmt)
    small = list(_chain(yuv, fmt, H, W, Hd, Wd))
    for split in (False, True):
        op, close = _op(species, Hd, Wd)
        pipe = FramePipeline(op, Hd, Wd, depth=3, split_compare=split)
        want = _run(pipe, small)
        if close:
            close()
        op, close = _op(species, Hd, Wd)
        pipe = FramePipeline(op, H, W, depth=3, split_compare=split, io_format="yuv", pix_fmt=fmt, scale=(Wd, Hd))
        assert (pipe.H, pipe.W, pipe.out_H, pipe.out_W) == (H, W, Hd, Wd)
        assert pipe.slots[0].h_in.array.nbytes == R.frame_size(fmt, H, W) and pipe.slots[0].h_out.array.nbytes == R.frame_size(fmt, Hd, Wd)
        got = _run(pipe, list(yuv))
        if close:
            close()
        for k in range(len(small)):
            assert got[k].shape == (R.frame_size(fmt, Hd, Wd),)
            assert np.array_equal(got[k], R.encode(want[k], fmt)), (species, fmt, split, k)


def test_scaled_pipeline_batch_4_equals_batch_1():
    from animal_vision_amd.pipeline import FramePipeline

    H, W, Hd, Wd, fmt = 96, 160, 48, 80, "nv12"
    yuv = list(R.encode(_frames(6, H, W, seed=2), fmt))
    for species in ("dog", "reindeer"):
        outs = []
        for batch in (1, 4):
            op, close = _op(species, Hd, Wd, batch)
            outs.append(_run(FramePipeline(op, H, W, depth=2, io_format="yuv", pix_fmt=fmt, scale=(Wd, Hd), batch=batch), yuv))
            if close:
                close()
        assert all(np.array_equal(a, b) for a, b in zip(*outs)), species


@pytest.mark.parametrize("io", ["rgb", "i420"])
def test_scaled_split_compare_has_the_scaled_size_and_the_scaled_original_on_the_left(io):
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.yuv import i420_to_rgb

    H, W, Hd, Wd = 97, 161, 64, 100
    rgb = _frames(3, H, W, seed=7)
    if io == "rgb":
        frames, small = list(rgb), [_resize(f, Hd, Wd) for f in rgb]
    else:
        yuv = R.encode(rgb, "yuv420p")
        frames, small = list(yuv), list(_chain(yuv, "yuv420p", H, W, Hd, Wd))
    want = _run(FramePipeline(_op("dog", Hd, Wd)[0], Hd, Wd, split_compare=True, labels=None), small)
    got = _run(FramePipeline(_op("dog", Hd, Wd)[0], H, W, split_compare=True, labels=None, io_format=io, scale=(Wd, Hd)), frames)
    for k in range(3):
        if io == "rgb":
            assert got[k].shape == (Hd, Wd, 3)
            assert np.array_equal(got[k], want[k])
            assert np.array_equal(got[k][:, : Wd // 2], small[k][:, : Wd // 2])  # the scaled original
            assert (got[k][:, Wd // 2] == 255).all()                            # the seam
        else:
            assert np.array_equal(got[k], R.encode(want[k], "yuv420p"))
            assert i420_to_rgb(got[k], Hd, Wd).shape == (Hd, Wd, 3)


def test_scaled_hdr_pipeline_equals_the_hdr_decode_then_the_resize():
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.yuv import yuv_hdr_to_rgb

    H, W, Hd, Wd, fmt = 96, 160, 48, 80, "p010le"
    yuv = R.random_payload(fmt, 5, H, W, seed=4)
    small = [_resize(f, Hd, Wd) for f in yuv_hdr_to_rgb(yuv, H, W, pix_fmt=fmt, transfer="pq")]
    want = _run(FramePipeline(_op("dog", Hd, Wd)[0], Hd, Wd), small)
    for batch in (1, 2):
        got = _run(FramePipeline(_op("dog", Hd, Wd)[0], H, W, io_format="yuv", pix_fmt=fmt, transfer="pq", scale=(Wd, Hd), batch=batch), list(yuv))
        for k in range(5):
            assert np.array_equal(got[k], R.encode(want[k], fmt, "bt709", "limited")), (batch, k)


def test_pipeline_without_scale_is_unchanged_and_scale_equal_to_the_size_is_the_plain_pipeline():
    from animal_vision_amd.pipeline import FramePipeline

    H, W, fmt = 32, 48, "nv12"
    yuv = list(R.encode(_frames(3, H, W, seed=1), fmt))
    plain = FramePipeline(_op("dog", H, W)[0], H, W, io_format="yuv", pix_fmt=fmt)
    assert plain.scale is None and (plain.out_H, plain.out_W) == (H, W) and plain.slots[0].d_full is None
    a = _run(plain, yuv)
    b = _run(FramePipeline(_op("dog", H, W)[0], H, W, io_format="yuv", pix_fmt=fmt, scale=(W, H)), yuv)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- run_video and the command ------------------------------------
def _write_raw(path, yuv):
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(yuv, np.uint8).tobytes())


def test_run_video_raw_nv12_scaled_world_1_and_2_byte_identical(tmp_path, oracle):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import run_video
    from animal_vision_amd.renderers import VideoRenderer

    H, W, Hd, Wd, fmt = 96, 160, 48, 80, "nv12"
    yuv = R.encode(_frames(7, H, W, seed=3), fmt)
    src = str(tmp_path / "in.yuv")
    _write_raw(src, yuv)
    for world in (1, 2):
        dst = str(tmp_path / f"out{world}.yuv")
        for rank in range(world):
            vr = VideoRenderer(read_path=src, write_path=dst, rank=rank, world=world, pix_fmt=fmt, size=(W, H), scale=(Wd, Hd))
            vr.open()
            assert vr.yuv_hw == (H, W) and vr.out_hw == (Hd, Wd) and vr.yuv_pix_fmt == fmt
            st = run_video(DichromatOp(Dog.SPEC), vr, rank=rank, world=world)
            vr.close()
            assert st.frames == len(range(rank, 7, world))
        if world > 1:
            vr.merge_shards()
    one = open(str(tmp_path / "out1.yuv"), "rb").read()
    assert len(one) == 7 * R.frame_size(fmt, Hd, Wd)  # the sink has the scaled size
    assert one == open(str(tmp_path / "out2.yuv"), "rb").read()
    got = np.frombuffer(one, np.uint8).reshape(7, R.frame_size(fmt, Hd, Wd))
    small = _chain(yuv, fmt, H, W, Hd, Wd)
    for k in range(7):
        want = oracle.dichromat_visualize(oracle.DICHROMATS["dog"], small[k])[1]
        assert np.array_equal(got[k], R.encode(want, fmt)), k


def test_get_image_returns_scaled_frames_for_every_source(tmp_path):
    from animal_vision_amd.renderers import VideoRenderer
    from animal_vision_amd.renderers.y4m import Y4MWriter, default_header
    from animal_vision_amd.yuv import yuv_hdr_to_rgb

    H, W, Hd, Wd = 97, 161, 64, 100
    rgb = _frames(2, H, W, seed=6)

    def frames_of(**kw):
        vr = VideoRenderer(scale=(Wd, Hd), **kw)
        vr.open()
        out = []
        while (f := vr.get_image()) is not None:
            out.append(f)
        vr.close()
        return out

    # raw
    yuv = R.encode(rgb, "p010le")
    _write_raw(str(tmp_path / "in.yuv"), yuv)
    got = frames_of(read_path=str(tmp_path / "in.yuv"), pix_fmt="p010le", size=(W, H))
    assert np.array_equal(np.stack(got), _chain(yuv, "p010le", H, W, Hd, Wd))
    # HDR: the HDR decode, then the resize
    got = frames_of(read_path=str(tmp_path / "in.yuv"), pix_fmt="p010le", size=(W, H), transfer="hlg")
    assert np.array_equal(np.stack(got), np.stack([_resize(f, Hd, Wd) for f in yuv_hdr_to_rgb(yuv, H, W, pix_fmt="p010le", transfer="hlg")]))
    # .y4m
    i420 = R.encode(rgb, "yuv420p")
    wr = Y4MWriter(str(tmp_path / "in.y4m"), default_header(W, H))
    for f in i420:
        wr.write(f)
    wr.close()
    got = frames_of(read_path=str(tmp_path / "in.y4m"))
    assert np.array_equal(np.stack(got), _chain(i420, "yuv420p", H, W, Hd, Wd))
    # .npy and synthetic: the resize alone
    np.save(str(tmp_path / "in.npy"), rgb)
    got = frames_of(read_path=str(tmp_path / "in.npy"))
    assert np.array_equal(np.stack(got), np.stack([_resize(f, Hd, Wd) for f in rgb]))
    got = frames_of(read_path=f"synthetic:{W}x{H}:2:structured")
    assert len(got) == 2 and got[0].shape == (Hd, Wd, 3)
    with pytest.raises(ValueError):
        VideoRenderer(read_path=str(tmp_path / "in.y4m"), scale=(W + 1, H)).open()


def test_cli_scale_raw_nv12_file_and_stdin_to_stdout(tmp_path, capsys):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.renderers import split_compose
    from animal_vision_amd.video import main

    H, W, Hd, Wd, fmt = 96, 160, 48, 80, "nv12"
    yuv = R.encode(_frames(4, H, W, seed=9), fmt)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "dog.yuv")
    _write_raw(src, yuv)
    small = _chain(yuv, fmt, H, W, Hd, Wd)
    args = ["--species", "Dog", "--split-compare", "--pix-fmt", fmt, "--size", f"{W}x{H}", "--scale", f"{Wd}x{Hd}"]
    assert main([src, dst] + args) == 0
    assert "4 frames" in capsys.readouterr().err
    got = np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(4, -1)
    assert got.shape[1] == R.frame_size(fmt, Hd, Wd)
    for k in range(4):
        want = split_compose(small[k], Dog().visualize(small[k])[1], left_label="Original", right_label="Transformed")
        assert np.array_equal(got[k], R.encode(want, fmt)), k
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "animal_vision_amd.video", "-", "-"] + args, input=open(src, "rb").read(), capture_output=True,
                         timeout=180, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    assert out.stdout == open(dst, "rb").read()
    assert b"4 frames" in out.stderr


def test_cli_scale_y4m_to_y4m_writes_the_scaled_header(tmp_path, capsys):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.renderers.y4m import Y4MReader, Y4MWriter, default_header
    from animal_vision_amd.video import main

    H, W, Hd, Wd = 96, 160, 48, 80
    i420 = R.encode(_frames(3, H, W, seed=12), "yuv420p")
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    wr = Y4MWriter(src, default_header(W, H))
    for f in i420:
        wr.write(f)
    wr.close()
    assert main([src, dst, "--species", "Dog", "--scale", f"{Wd}x{Hd}"]) == 0
    capsys.readouterr()
    rd = Y4MReader(dst)
    assert (rd.header.width, rd.header.height) == (Wd, Hd) and rd.total_frames == 3
    small = _chain(i420, "yuv420p", H, W, Hd, Wd)
    for k in range(3):
        assert np.array_equal(rd.read(), R.encode(Dog().visualize(small[k])[1], "yuv420p")), k
    rd.close()
