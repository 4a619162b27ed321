"""GPU: the YUV 4:2:0 <-> RGB kernels (csrc/yuv.hip) bit for bit against the NumPy restatement of DESIGN §4.8
(tests/_yuv_ref.py), FramePipeline(io_format="i420") against the RGB pipeline put through that restatement, run_video and the
`video` command from .y4m to .y4m (sharded and merged, per-frame route, and through stdin / stdout)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _yuv_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

COMBOS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]


def _yuv_frames(n, H, W, seed=0, matrix="bt601", rng="limited"):
    """I420 payloads of real picture content: the structured synthetic frames through the encode restatement."""
    from animal_vision_amd.synthetic import structured_frame

    return R.encode(np.stack([structured_frame(seed + k, H, W) for k in range(n)]), matrix, rng)


# ---------------------------------------------------------------- kernels ------------------------------------------------------
@pytest.mark.parametrize("matrix,rng", COMBOS)
def test_decode_every_triple_bit_identical(matrix, rng):
    """64 frames of 512 x 512: chroma block b carries (U, V) = (b & 255, b >> 8), so the 256 x 256 chroma plane holds all 65536
    pairs, and the four luma samples of that block in frame k are 4k .. 4k + 3 -- every (Y, U, V) triple once, one launch."""
    from animal_vision_amd.yuv import i420_to_rgb

    H = W = 512
    b = np.arange(1 << 16, dtype=np.int64).reshape(256, 256)
    U, V = (b & 255).astype(np.uint8), (b >> 8).astype(np.uint8)
    j = np.array([[0, 1], [2, 3]], np.int64)
    buf = np.empty((64, R.i420_size(H, W)), np.uint8)
    for k in range(64):
        buf[k, : H * W] = np.tile(4 * k + j, (256, 256)).reshape(-1)
        buf[k, H * W: H * W + 65536] = U.reshape(-1)
        buf[k, H * W + 65536:] = V.reshape(-1)
    got = i420_to_rgb(buf, H, W, matrix=matrix, range=rng)
    assert got.shape == (64, H, W, 3)
    assert np.array_equal(got, R.decode(buf, H, W, matrix, rng))


@pytest.mark.parametrize("H,W", [(1080, 1920), (2160, 3840), (97, 161), (64, 40), (1, 1), (3, 18)])
def test_encode_bit_identical_and_batch_equals_frame_by_frame(H, W):
    from animal_vision_amd.yuv import rgb_to_i420

    n = 1 if H * W > 4_000_000 else 3
    rgb = np.random.default_rng(H * 7 + W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    for matrix, rng in COMBOS if H * W < 4_000_000 else COMBOS[:1]:
        got = rgb_to_i420(rgb, matrix=matrix, range=rng)
        assert got.shape == (n, R.i420_size(H, W))
        assert np.array_equal(got, R.encode(rgb, matrix, rng)), (H, W, matrix, rng)
        for k in range(n):
            assert np.array_equal(rgb_to_i420(rgb[k], matrix=matrix, range=rng), got[k])


@pytest.mark.parametrize("H,W", [(1080, 1920), (2160, 3840), (97, 161), (64, 40)])
def test_decode_sizes_bit_identical_and_batch_equals_frame_by_frame(H, W):
    from animal_vision_amd.yuv import i420_to_rgb

    n = 1 if H * W > 4_000_000 else 3
    buf = np.random.default_rng(W).integers(0, 256, (n, R.i420_size(H, W)), dtype=np.uint8)
    got = i420_to_rgb(buf, H, W, matrix="bt709", range="limited")
    assert np.array_equal(got, R.decode(buf, H, W, "bt709", "limited"))
    for k in range(n):
        assert np.array_equal(i420_to_rgb(buf[k], H, W, matrix="bt709", range="limited"), got[k])


@pytest.mark.parametrize("matrix,rng", COMBOS)
def test_greys_encode_to_exactly_128(matrix, rng):
    from animal_vision_amd.yuv import i420_to_rgb, rgb_to_i420

    H, W = 32, 256
    grey = np.repeat(np.arange(256, dtype=np.uint8), 3)[None, :].repeat(H, 0).reshape(H, W, 3)
    enc = rgb_to_i420(grey, matrix=matrix, range=rng)
    assert (enc[H * W:] == 128).all()
    if rng == "full":  # full range greys survive the round trip exactly
        assert np.array_equal(i420_to_rgb(enc, H, W, matrix=matrix, range=rng), grey)


def test_bad_arguments_raise():
    from animal_vision_amd._lib import AVX_ERR_INVALID, lib
    from animal_vision_amd.runtime import get_context
    from animal_vision_amd.yuv import i420_to_rgb

    ctx = get_context()
    d = ctx.malloc(1024)
    try:
        for args in ((d.ptr, d.ptr, 1, 8, 8, 0, 0), (d.ptr, 0, 1, 8, 8, 0, 0), (d.ptr, d.ptr + 512, 0, 8, 8, 0, 0),
                     (d.ptr, d.ptr + 512, 1, 8, 8, 2, 0), (d.ptr, d.ptr + 512, 1, 8, 8, 0, 2), (d.ptr, d.ptr + 512, 1, -8, 8, 0, 0)):
            for fn in (lib.avx_i420_to_rgb_u8, lib.avx_rgb_to_i420_u8):
                assert fn(ctx._h, *args, ctx.stream) == AVX_ERR_INVALID, args
                assert lib.avx_last_error(ctx._h).decode().startswith(fn.__name__)
    finally:
        d.free()
    with pytest.raises(ValueError):
        i420_to_rgb(np.zeros(10, np.uint8), 4, 4)
    with pytest.raises(ValueError):
        i420_to_rgb(np.zeros(24, np.uint8), 4, 4, matrix="bt2020")


# ---------------------------------------------------------------- FramePipeline(io_format="i420") -------------------------------
def _run(pipe, frames):
    got = {}
    pipe.run(((i, f) for i, f in enumerate(frames)), lambda i, o: got.__setitem__(i, o))
    pipe.close()
    return [got[i] for i in range(len(frames))]


@pytest.mark.parametrize("species,H,W", [("dog", 96, 160), ("dog", 97, 161), ("honeybee", 96, 160), ("reindeer", 96, 160)])
def test_i420_pipeline_equals_rgb_pipeline_through_the_encode(oracle, species, H, W):
    from animal_vision_amd.animals import Dog, HoneyBee, Reindeer
    from animal_vision_amd.animals._uv_species import SpeciesStreamOp
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import FramePipeline

    yuv = _yuv_frames(5, H, W, seed=11)
    rgb = list(R.decode(yuv, H, W))
    for split in (False, True):
        outs = {}
        for fmt in ("rgb", "i420"):
            if species == "dog":
                op, close = DichromatOp(Dog.SPEC), None
            elif species == "honeybee":
                op, close = HoneyBee()._operator(), None
            else:
                op = SpeciesStreamOp(Reindeer(), H, W, depth=3)
                close = op.close
            pipe = FramePipeline(op, H, W, depth=3, split_compare=split, io_format=fmt)
            assert pipe.slots[0].h_in.array.nbytes == (H * W * 3 if fmt == "rgb" else R.i420_size(H, W))
            outs[fmt] = _run(pipe, rgb if fmt == "rgb" else list(yuv))
            if close:
                close()
        for k in range(len(rgb)):
            assert np.array_equal(outs["i420"][k], R.encode(outs["rgb"][k])), (species, split, k)
            if species == "dog" and not split:  # the RGB path stays bit-exact against the oracle
                assert np.array_equal(outs["rgb"][k], oracle.dichromat_visualize(oracle.DICHROMATS["dog"], rgb[k])[1]), k


def test_pipeline_io_format_argument():
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import FramePipeline

    with pytest.raises(ValueError):
        FramePipeline(DichromatOp(Dog.SPEC), 16, 16, io_format="nv12")
    pipe = FramePipeline(DichromatOp(Dog.SPEC), 16, 16, depth=1, io_format="i420")
    try:
        with pytest.raises(ValueError):
            pipe.run(iter([(0, np.zeros((16, 16, 3), np.uint8))]), lambda i, o: None)
    finally:
        pipe.close()


# ---------------------------------------------------------------- run_video and the command ------------------------------------
def _write_y4m(path, yuv, H, W, header="F25:1 Ip A1:1 C420jpeg XYSCSS=420JPEG"):
    with open(path, "wb") as f:
        f.write(R.y4m_bytes(list(yuv), H, W, header=header))


def _read_y4m(path):
    from animal_vision_amd.renderers.y4m import Y4MReader

    rd = Y4MReader(path)
    out = []
    while (f := rd.read()) is not None:
        out.append(f)
    hdr = rd.header
    rd.close()
    return hdr, out


def test_run_video_y4m_world_1_and_2_byte_identical(tmp_path, oracle):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import run_video
    from animal_vision_amd.renderers import VideoRenderer

    H, W = 96, 160
    yuv = _yuv_frames(7, H, W, seed=3)
    src = str(tmp_path / "in.y4m")
    _write_y4m(src, yuv, H, W)
    for world in (1, 2):
        dst = str(tmp_path / f"out{world}.y4m")
        for rank in range(world):
            vr = VideoRenderer(read_path=src, write_path=dst, rank=rank, world=world)
            vr.open()
            st = run_video(DichromatOp(Dog.SPEC), vr, rank=rank, world=world)
            vr.close()
            assert st.frames == len(range(rank, 7, world))
        if world > 1:
            vr.merge_shards()
    one = open(str(tmp_path / "out1.y4m"), "rb").read()
    assert one == open(str(tmp_path / "out2.y4m"), "rb").read()
    hdr, frames = _read_y4m(str(tmp_path / "out1.y4m"))
    assert hdr.encode() == f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C420jpeg XYSCSS=420JPEG\n".encode()
    for k, f in enumerate(frames):
        want = oracle.dichromat_visualize(oracle.DICHROMATS["dog"], R.decode(yuv[k], H, W))[1]
        assert np.array_equal(f, R.encode(want)), k


def test_get_image_and_rgb_render_convert_on_the_device(tmp_path):
    from animal_vision_amd.renderers import VideoRenderer

    H, W = 97, 161
    yuv = _yuv_frames(3, H, W, seed=5, matrix="bt709", rng="full")
    src = str(tmp_path / "full.y4m")
    _write_y4m(src, yuv, H, W, header="F30:1 Ip XCOLORRANGE=FULL")
    vr = VideoRenderer(read_path=src, write_path=str(tmp_path / "o.y4m"), matrix="bt709")
    vr.open()
    assert vr.yuv_range == "full"
    k = 0
    while (f := vr.get_image()) is not None:
        assert f.shape == (H, W, 3) and np.array_equal(f, R.decode(yuv[k], H, W, "bt709", "full"))
        vr.render(f)
        k += 1
    vr.close()
    hdr, frames = _read_y4m(str(tmp_path / "o.y4m"))
    assert hdr.full_range and k == 3
    for k, f in enumerate(frames):
        assert np.array_equal(f, R.encode(R.decode(yuv[k], H, W, "bt709", "full"), "bt709", "full"))


def test_cli_dog_streamed_and_cat_per_frame(tmp_path, capsys):
    from animal_vision_amd.animals import Cat, Dog
    from animal_vision_amd.renderers import split_compose
    from animal_vision_amd.video import main

    H, W = 96, 160
    yuv = _yuv_frames(4, H, W, seed=9)
    src = str(tmp_path / "in.y4m")
    _write_y4m(src, yuv, H, W)
    rgb = R.decode(yuv, H, W)

    dst = str(tmp_path / "dog.y4m")
    assert main([src, dst, "--species", "Dog", "--split-compare"]) == 0
    assert "4 frames" in capsys.readouterr().err
    _, frames = _read_y4m(dst)
    for k, f in enumerate(frames):
        want = split_compose(rgb[k], Dog().visualize(rgb[k])[1], left_label="Original", right_label="Transformed")
        assert np.array_equal(f, R.encode(want)), k

    dst = str(tmp_path / "cat.y4m")
    assert main([src, dst, "--species", "Cat", "--split-compare", "--no-labels"]) == 0
    _, frames = _read_y4m(dst)
    assert len(frames) == 4
    for k, f in enumerate(frames):
        base, out = Cat().visualize(rgb[k])
        assert not np.array_equal(base, rgb[k])  # Cat's baseline is the zoomed frame, not the input
        assert np.array_equal(f, R.encode(split_compose(base, out))), k


@pytest.mark.parametrize("name", ["ReinDeer", "GoldFish"])
def test_cli_uv_species_split_compare_left_half_is_its_baseline(tmp_path, name):
    """A plane-program species streams through run_video, and its split frame is composed against visualize()'s own baseline
    (the panorama-warped input), not the raw input: the reference's render_split_compare(baseline_out, out)."""
    from animal_vision_amd.gallery import species_class
    from animal_vision_amd.renderers import split_compose
    from animal_vision_amd.video import main, route

    H, W = 96, 160
    yuv = _yuv_frames(3, H, W, seed=17)
    src = str(tmp_path / "in.y4m")
    _write_y4m(src, yuv, H, W)
    rgb = R.decode(yuv, H, W)
    sp = species_class(name)()
    assert route(sp) == "plane"
    dst = str(tmp_path / "uv.y4m")
    assert main([src, dst, "--species", name, "--split-compare"]) == 0
    _, frames = _read_y4m(dst)
    assert len(frames) == 3
    for k, f in enumerate(frames):
        base, out = sp.visualize(rgb[k])
        assert not np.array_equal(base, rgb[k])  # the baseline is widened and centre-cropped: a test against the input would differ
        want = split_compose(base, out, left_label="Original", right_label="Transformed")
        assert np.array_equal(f, R.encode(want)), (name, k)


def test_cli_pipes_stdin_to_stdout(tmp_path):
    from animal_vision_amd.video import main

    H, W = 64, 96
    yuv = _yuv_frames(3, H, W, seed=13)
    src = str(tmp_path / "in.y4m")
    _write_y4m(src, yuv, H, W)
    ref = str(tmp_path / "ref.y4m")
    assert main([src, ref, "--species", "Wolf", "--split-compare"]) == 0
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "animal_vision_amd.video", "-", "-", "--species", "Wolf", "--split-compare"],
                         input=open(src, "rb").read(), capture_output=True, timeout=180, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    assert out.stdout == open(ref, "rb").read()
    assert b"3 frames" in out.stderr
