"""GPU: the HDR decode kernels (csrc/yuv_hdr.hip) against the float64 definition of DESIGN §4.10 (tests/_hdr_ref.py), within one
output code, for every 10-bit format on the block path and the vector path; the two paths against each other byte for byte;
p010le against yuv420p10le; the exact anchors; the C entry point's argument checks; FramePipeline(transfer=...) and the `video`
command against the composition built by hand from the device's own decode."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _hdr_ref as H
import _rawyuv_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

# odd sizes, one pixel, and sizes the 4:2:0 formats take on the vector path (W % 16 == 0, H even): (64, 40) is not one, (32, 48) is
SIZES = [(1, 1), (3, 18), (97, 161), (64, 40), (32, 48)]


def _diff(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


def _frames(n, Hh, W, seed=0):
    from animal_vision_amd.synthetic import structured_frame

    return np.stack([structured_frame(seed + k, Hh, W) for k in range(n)])


# ---------------------------------------------------------------- kernels ------------------------------------------------------
@pytest.mark.parametrize("transfer", H.TRANSFERS)
@pytest.mark.parametrize("fmt", H.FORMATS)
def test_decode_within_one_code_and_batch_equals_frame_by_frame(fmt, transfer):
    from animal_vision_amd.yuv import yuv_hdr_to_rgb

    for k, (Hh, W) in enumerate(SIZES):
        rng, tm = H.RANGES[k % 2], H.TONEMAPS[(k // 2 + H.FORMATS.index(fmt)) % 2]
        buf = R.random_payload(fmt, 3, Hh, W, seed=Hh * 7 + W)
        got = yuv_hdr_to_rgb(buf, Hh, W, pix_fmt=fmt, transfer=transfer, range=rng, tonemap=tm)
        assert got.shape == (3, Hh, W, 3) and got.dtype == np.uint8
        assert _diff(got, H.decode(buf, fmt, Hh, W, transfer, rng, tm)) <= 1, (fmt, transfer, Hh, W, rng, tm)
        for j in range(3):
            assert np.array_equal(yuv_hdr_to_rgb(buf[j], Hh, W, pix_fmt=fmt, transfer=transfer, range=rng, tonemap=tm), got[j]), (fmt, Hh, W, j)


@pytest.mark.parametrize("transfer", H.TRANSFERS)
@pytest.mark.parametrize("fmt", ["yuv420p10le", "p010le"])
def test_vector_path_equals_block_path_byte_for_byte(fmt, transfer):
    """The same (32, 48) payload from an aligned buffer (vector path) and from ptr + 2 (not 16-byte aligned: block path)."""
    from animal_vision_amd.runtime import get_context
    from animal_vision_amd.yuv import yuv_hdr_to_rgb_device

    Hh, W, n = 32, 48, 2
    buf = R.random_payload(fmt, n, Hh, W, seed=5)
    ctx = get_context()
    d_in, d_out = ctx.malloc(buf.nbytes + 16), ctx.malloc(n * Hh * W * 3)
    outs = []
    try:
        assert d_in.ptr % 16 == 0 and d_out.ptr % 16 == 0
        for off in (0, 2):
            v = d_in.view(off, buf.nbytes)
            ctx.upload(buf, v)
            ctx.memset(d_out, 0)
            yuv_hdr_to_rgb_device(ctx, fmt, v, d_out, n, Hh, W, transfer=transfer)
            outs.append(ctx.download(d_out, (n, Hh, W, 3), np.uint8))
    finally:
        d_in.free()
        d_out.free()
    assert np.array_equal(outs[0], outs[1])
    assert _diff(outs[0], H.decode(buf, fmt, Hh, W, transfer)) <= 1


@pytest.mark.parametrize("Hh,W", [(97, 161), (32, 48)])
def test_p010le_equals_yuv420p10le_on_the_same_samples(Hh, W):
    from animal_vision_amd.yuv import yuv_hdr_to_rgb

    p010 = R.random_payload("p010le", 2, Hh, W, seed=Hh)  # random low 6 bits: ignored on read
    assert (p010[:, 0::2] & 63).any()
    planar = R.join_planes(*R.split_planes(p010, "p010le", Hh, W), "yuv420p10le")
    for transfer in H.TRANSFERS:
        assert np.array_equal(yuv_hdr_to_rgb(p010, Hh, W, pix_fmt="p010le", transfer=transfer),
                              yuv_hdr_to_rgb(planar, Hh, W, pix_fmt="yuv420p10le", transfer=transfer))


def _row_444(t):
    """(n, 3) triples of (Y, U, V) as a 1-row yuv444p10le frame."""
    return R.join_planes(t[None, None, :, 0], t[None, None, :, 1], t[None, None, :, 2], "yuv444p10le")[0]


@pytest.mark.parametrize("transfer", H.TRANSFERS)
def test_lattice_of_extremes_and_the_exact_anchors(transfer):
    from animal_vision_amd.yuv import yuv_hdr_to_rgb

    t = H.lattice()
    for rng in H.RANGES:
        for tm in H.TONEMAPS:
            got = yuv_hdr_to_rgb(_row_444(t), 1, len(t), pix_fmt="yuv444p10le", transfer=transfer, range=rng, tonemap=tm)[0]
            assert _diff(got, H.decode_px(t[:, 0], t[:, 1], t[:, 2], transfer, rng, tm)) <= 1, (transfer, rng, tm)
            # every neutral Y: R = G = B exactly, and within one code of the definition; black is exactly black
            n = np.stack([np.arange(1024), np.full(1024, 512), np.full(1024, 512)], -1)
            got = yuv_hdr_to_rgb(_row_444(n), 1, 1024, pix_fmt="yuv444p10le", transfer=transfer, range=rng, tonemap=tm)[0]
            assert (got[:, 0] == got[:, 1]).all() and (got[:, 1] == got[:, 2]).all(), (transfer, rng, tm)
            assert _diff(got, H.decode_px(n[:, 0], n[:, 1], n[:, 2], transfer, rng, tm)) <= 1
            assert np.array_equal(got[0 if rng == "full" else 64], [0, 0, 0]) and np.array_equal(got[1023], [255, 255, 255])
    # the neutral anchors hold through the subsampled formats' block and vector kernels too
    Hh, W = 32, 64
    Y = np.arange(Hh * W).reshape(1, Hh, W) % 1024
    C = np.full((1, Hh // 2, W // 2), 512)
    for fmt in ("p010le", "yuv420p10le"):
        got = yuv_hdr_to_rgb(R.join_planes(Y, C, C, fmt)[0], Hh, W, pix_fmt=fmt, transfer=transfer)
        assert (got[..., 0] == got[..., 1]).all() and (got[..., 1] == got[..., 2]).all() and (got[Y[0] == 64] == 0).all()


def test_one_1080p_p010le_frame_pq():
    from animal_vision_amd.yuv import yuv_hdr_to_rgb

    Hh, W = 1080, 1920
    buf = R.random_payload("p010le", 1, Hh, W, seed=1080)[0]
    got = yuv_hdr_to_rgb(buf, Hh, W, pix_fmt="p010le", transfer="pq")
    assert _diff(got, H.decode(buf, "p010le", Hh, W, "pq")) <= 1


def test_bad_arguments_return_invalid_with_the_name_first():
    from animal_vision_amd._lib import AVX_ERR_INVALID, AVX_OK, lib
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    d = ctx.malloc(8192)
    a, b = d.ptr, d.ptr + 4096
    inf, nan = float("inf"), float("nan")
    ok = (8, a, b, 1, 8, 8, 0, 1, 1, 1000.0, 203.0)  # fmt, yuv, rgb, n, H, W, full_range, transfer, tonemap, peak_nits, sdr_white

    def but(**kw):
        names = ("fmt", "yuv", "rgb", "n", "H", "W", "full_range", "transfer", "tonemap", "peak_nits", "sdr_white")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    try:
        assert lib.avx_yuv_hdr_to_rgb_u8(ctx._h, *ok, ctx.stream) == AVX_OK
        ctx.sync()
        bad = [but(fmt=0), but(fmt=1), but(fmt=2), but(fmt=3), but(fmt=4), but(fmt=9), but(fmt=-1),  # 8-bit formats, gray, no format
               but(transfer=0), but(transfer=3), but(tonemap=-1), but(tonemap=2),
               but(peak_nits=203.0), but(peak_nits=100.0), but(peak_nits=inf), but(peak_nits=nan), but(sdr_white=0.0), but(sdr_white=-203.0),
               but(sdr_white=nan), but(sdr_white=inf), but(peak_nits=-5.0, sdr_white=-10.0),
               but(yuv=0), but(rgb=0), but(rgb=a), but(rgb=a + 64), but(yuv=a + 1),
               but(n=0), but(H=0), but(W=-8), but(H=1 << 16), but(full_range=2)]
        for args in bad:
            assert lib.avx_yuv_hdr_to_rgb_u8(ctx._h, *args, ctx.stream) == AVX_ERR_INVALID, args
            assert lib.avx_last_error(ctx._h).decode().startswith("avx_yuv_hdr_to_rgb_u8"), args
        assert lib.avx_yuv_hdr_to_rgb_u8(None, *ok, ctx.stream) == AVX_ERR_INVALID
        # the fixed-point entry points keep refusing the BT.2020 matrix code
        assert lib.avx_yuv_to_rgb_u8(ctx._h, 8, a, b, 1, 8, 8, 2, 0, ctx.stream) == AVX_ERR_INVALID
        assert lib.avx_rgb_to_yuv_u8(ctx._h, 8, b, a, 1, 8, 8, 2, 0, ctx.stream) == AVX_ERR_INVALID
    finally:
        d.free()


# ---------------------------------------------------------------- FramePipeline --------------------------------------------------
def _run(pipe, frames):
    got = {}
    pipe.run(((i, f) for i, f in enumerate(frames)), lambda i, o: got.__setitem__(i, o))
    pipe.close()
    return [got[i] for i in range(len(frames))]


@pytest.mark.parametrize("Hh,W", [(96, 160), (97, 161)])
def test_hdr_pipeline_equals_the_composition_by_hand(Hh, W):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.yuv import rgb_to_yuv, yuv_hdr_to_rgb, yuv_to_rgb

    fmt = "p010le"
    yuv = R.random_payload(fmt, 5, Hh, W, seed=W)
    for split in (False, True):
        pipe = FramePipeline(DichromatOp(Dog.SPEC), Hh, W, depth=3, split_compare=split, io_format="yuv", pix_fmt=fmt, transfer="pq")
        assert pipe.out_matrix == "bt709" and pipe.slots[0].h_in.array.nbytes == R.frame_size(fmt, Hh, W)
        got = _run(pipe, list(yuv))
        sdr = yuv_hdr_to_rgb(yuv, Hh, W, pix_fmt=fmt, transfer="pq")  # the device's own decode: this test pins the plumbing
        want = _run(FramePipeline(DichromatOp(Dog.SPEC), Hh, W, depth=3, split_compare=split), list(sdr))
        for k in range(len(yuv)):
            assert np.array_equal(got[k], rgb_to_yuv(want[k], pix_fmt=fmt, matrix="bt709")), (split, k)
    # other settings reach the decode and the encode
    kw = dict(transfer="hlg", tonemap="clip", peak_nits=4000.0, sdr_white=100.0, out_matrix="bt601", yuv_range="full")
    got = _run(FramePipeline(DichromatOp(Dog.SPEC), Hh, W, depth=2, io_format="yuv", pix_fmt=fmt, batch=2, **kw), list(yuv))
    sdr = yuv_hdr_to_rgb(yuv, Hh, W, pix_fmt=fmt, transfer="hlg", tonemap="clip", peak_nits=4000.0, sdr_white=100.0, range="full")
    want = _run(FramePipeline(DichromatOp(Dog.SPEC), Hh, W, depth=2), list(sdr))
    for k in range(len(yuv)):
        assert np.array_equal(got[k], rgb_to_yuv(want[k], pix_fmt=fmt, matrix="bt601", range="full")), k
    # transfer=None: every byte as without the new arguments
    for matrix in ("bt601", "bt709"):
        got = _run(FramePipeline(DichromatOp(Dog.SPEC), Hh, W, depth=3, io_format="yuv", pix_fmt=fmt, matrix=matrix, transfer=None), list(yuv))
        sdr = yuv_to_rgb(yuv, Hh, W, pix_fmt=fmt, matrix=matrix)
        want = _run(FramePipeline(DichromatOp(Dog.SPEC), Hh, W, depth=3), list(sdr))
        for k in range(len(yuv)):
            assert np.array_equal(got[k], rgb_to_yuv(want[k], pix_fmt=fmt, matrix=matrix)), (matrix, k)


def test_video_renderer_get_image_returns_the_tone_mapped_frame(tmp_path):
    from animal_vision_amd.renderers import VideoRenderer
    from animal_vision_amd.yuv import rgb_to_yuv, yuv_hdr_to_rgb

    Hh, W, fmt = 33, 50, "yuv422p10le"
    yuv = R.random_payload(fmt, 2, Hh, W, seed=8)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "out.yuv")
    with open(src, "wb") as f:
        f.write(yuv.tobytes())
    vr = VideoRenderer(read_path=src, write_path=dst, pix_fmt=fmt, size=(W, Hh), transfer="hlg", tonemap="clip", write_pix_fmt="nv12")
    vr.open()
    assert vr.yuv_hw is None
    sdr = yuv_hdr_to_rgb(yuv, Hh, W, pix_fmt=fmt, transfer="hlg", tonemap="clip")
    for k in range(2):
        f = vr.get_image()
        assert np.array_equal(f, sdr[k])
        vr.render(f)
    assert vr.get_image() is None
    vr.close()
    assert open(dst, "rb").read() == rgb_to_yuv(sdr, pix_fmt="nv12", matrix="bt709").tobytes()


# ---------------------------------------------------------------- the command ----------------------------------------------------
def test_cli_p010le_hlg_through_a_child_process(tmp_path):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.yuv import rgb_to_yuv, yuv_hdr_to_rgb

    Hh, W, fmt = 64, 96, "p010le"
    yuv = R.random_payload(fmt, 4, Hh, W, seed=9)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "dog.yuv")
    with open(src, "wb") as f:
        f.write(yuv.tobytes())
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "animal_vision_amd.video", src, dst, "--species", "Dog", "--pix-fmt", fmt, "--size", f"{W}x{Hh}",
                          "--transfer", "hlg"], capture_output=True, timeout=180, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    assert b"4 frames" in out.stderr
    raw = open(dst, "rb").read()
    assert len(raw) == 4 * R.frame_size(fmt, Hh, W)
    got = np.frombuffer(raw, np.uint8).reshape(4, -1)
    sdr = yuv_hdr_to_rgb(yuv[0], Hh, W, pix_fmt=fmt, transfer="hlg")
    assert np.array_equal(got[0], rgb_to_yuv(Dog().visualize(sdr)[1], pix_fmt=fmt, matrix="bt709"))
