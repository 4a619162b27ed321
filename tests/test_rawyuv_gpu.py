"""GPU: the raw pixel format kernels (csrc/yuv_raw.hip) bit for bit against the NumPy restatement of DESIGN §4.9
(tests/_rawyuv_ref.py) for every format, on the block path and the vector path; yuv420p against the I420 entry points; p010le
against yuv420p10le; FramePipeline(io_format="yuv") against the RGB pipeline put through the restatement; run_video and the
`video` command from raw video to raw video (sharded and merged, and through stdin / stdout)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _rawyuv_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

FMTS = list(R.FORMATS)
# odd sizes, one pixel, and sizes the 4:2:0 formats take on the vector path (W % 16 == 0, H even): (64, 40) is not one, (32, 48) is
SIZES = [(1, 1), (3, 18), (97, 161), (64, 40), (32, 48)]
VEC_FMTS = ["nv12", "p010le", "yuv420p10le"]


def _frames(n, H, W, seed=0):
    from animal_vision_amd.synthetic import structured_frame

    return np.stack([structured_frame(seed + k, H, W) for k in range(n)])


# ---------------------------------------------------------------- kernels ------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_bit_identical_and_batch_equals_frame_by_frame(fmt):
    from animal_vision_amd.yuv import yuv_to_rgb

    for k, (H, W) in enumerate(SIZES):
        matrix, rng = R.COMBOS[k % 4]
        buf = R.random_payload(fmt, 3, H, W, seed=H * 7 + W)
        got = yuv_to_rgb(buf, H, W, pix_fmt=fmt, matrix=matrix, range=rng)
        assert got.shape == (3, H, W, 3) and got.dtype == np.uint8
        assert np.array_equal(got, R.decode(buf, fmt, H, W, matrix, rng)), (fmt, H, W, matrix, rng)
        for j in range(3):
            assert np.array_equal(yuv_to_rgb(buf[j], H, W, pix_fmt=fmt, matrix=matrix, range=rng), got[j]), (fmt, H, W, j)


@pytest.mark.parametrize("fmt", FMTS)
def test_encode_bit_identical_and_batch_equals_frame_by_frame(fmt):
    from animal_vision_amd.yuv import rgb_to_yuv

    for k, (H, W) in enumerate(SIZES):
        matrix, rng = R.COMBOS[(k + 1) % 4]
        rgb = np.random.default_rng(H * 11 + W).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        got = rgb_to_yuv(rgb, pix_fmt=fmt, matrix=matrix, range=rng)
        assert got.shape == (3, R.frame_size(fmt, H, W)) and got.dtype == np.uint8
        assert np.array_equal(got, R.encode(rgb, fmt, matrix, rng)), (fmt, H, W, matrix, rng)
        for j in range(3):
            assert np.array_equal(rgb_to_yuv(rgb[j], pix_fmt=fmt, matrix=matrix, range=rng), got[j]), (fmt, H, W, j)


@pytest.mark.parametrize("fmt", VEC_FMTS)
def test_one_1080p_frame_bit_identical(fmt):
    from animal_vision_amd.yuv import rgb_to_yuv, yuv_to_rgb

    H, W = 1080, 1920
    buf = R.random_payload(fmt, 1, H, W, seed=1080)[0]
    assert np.array_equal(yuv_to_rgb(buf, H, W, pix_fmt=fmt, matrix="bt709", range="limited"), R.decode(buf, fmt, H, W, "bt709", "limited"))
    rgb = np.random.default_rng(1920).integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert np.array_equal(rgb_to_yuv(rgb, pix_fmt=fmt, matrix="bt709", range="limited"), R.encode(rgb, fmt, "bt709", "limited"))


@pytest.mark.parametrize("matrix,rng", R.COMBOS)
def test_10bit_decode_every_luma_times_a_chroma_lattice(matrix, rng):
    """One yuv444p10le frame of 1024 x 4096: row y carries Y = y, column x the (U, V) pair x of a 64 x 64 lattice that holds 0,
    511, 512, 513 and 1023 -- all 1024 luma values against 4096 chroma pairs, one launch."""
    from animal_vision_amd.yuv import yuv_to_rgb

    vals = np.array(sorted((set(range(0, 1024, 17)) - {17}) | {511, 512, 513, 1023}))
    assert len(vals) == 64 and {0, 511, 512, 513, 1023} <= set(vals.tolist())
    H, W = 1024, 4096
    Y = np.broadcast_to(np.arange(H)[:, None], (H, W))
    U = np.broadcast_to(np.repeat(vals, 64)[None, :], (H, W))
    V = np.broadcast_to(np.tile(vals, 64)[None, :], (H, W))
    buf = R.join_planes(Y[None], U[None], V[None], "yuv444p10le")[0]
    got = yuv_to_rgb(buf, H, W, pix_fmt="yuv444p10le", matrix=matrix, range=rng)
    assert np.array_equal(got, np.stack(R.decode_px(Y, U, V, matrix, rng, 10), -1))


@pytest.mark.parametrize("H,W", [(97, 161), (64, 40), (32, 48), (1, 1)])
def test_yuv420p_equals_the_i420_entry_points(H, W):
    from animal_vision_amd.yuv import i420_to_rgb, rgb_to_i420, rgb_to_yuv, yuv_to_rgb

    for matrix, rng in R.COMBOS:
        buf = R.random_payload("yuv420p", 2, H, W, seed=W)
        assert np.array_equal(yuv_to_rgb(buf, H, W, pix_fmt="yuv420p", matrix=matrix, range=rng), i420_to_rgb(buf, H, W, matrix=matrix, range=rng))
        rgb = np.random.default_rng(H).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        assert np.array_equal(rgb_to_yuv(rgb, pix_fmt="yuv420p", matrix=matrix, range=rng), rgb_to_i420(rgb, matrix=matrix, range=rng))


@pytest.mark.parametrize("H,W", [(97, 161), (32, 48)])
def test_p010le_is_yuv420p10le_interleaved_and_shifted(H, W):
    from animal_vision_amd.yuv import rgb_to_yuv, yuv_to_rgb

    p010 = R.random_payload("p010le", 2, H, W, seed=H)  # random low 6 bits: ignored on read
    planar = R.join_planes(*R.split_planes(p010, "p010le", H, W), "yuv420p10le")
    assert np.array_equal(yuv_to_rgb(p010, H, W, pix_fmt="p010le"), yuv_to_rgb(planar, H, W, pix_fmt="yuv420p10le"))
    rgb = _frames(2, H, W, seed=4)
    enc = rgb_to_yuv(rgb, pix_fmt="p010le")
    assert (enc[:, 0::2] & 63 == 0).all()  # the low 6 bits of every sample are written as zero
    want = R.split_planes(rgb_to_yuv(rgb, pix_fmt="yuv420p10le"), "yuv420p10le", H, W)
    assert all(np.array_equal(a, b) for a, b in zip(R.split_planes(enc, "p010le", H, W), want))


def test_gray_decodes_with_neutral_chroma_and_greys_encode_neutral():
    from animal_vision_amd.yuv import rgb_to_yuv, yuv_to_rgb

    H, W = 32, 256
    grey = np.repeat(np.arange(256, dtype=np.uint8), 3)[None, :].repeat(H, 0).reshape(H, W, 3)
    for fmt in ("nv12", "yuv422p", "yuv444p10le", "p010le", "yuv420p10le"):
        _, U, V = R.split_planes(rgb_to_yuv(grey, pix_fmt=fmt, range="full"), fmt, H, W)
        c = 1 << (R.depth_of(fmt) - 1)
        assert (U == c).all() and (V == c).all(), fmt
    y = rgb_to_yuv(grey, pix_fmt="gray", range="full")
    assert y.shape == (H * W,) and np.array_equal(yuv_to_rgb(y, H, W, pix_fmt="gray", range="full"), grey)


def test_bad_arguments_return_invalid():
    from animal_vision_amd._lib import AVX_ERR_INVALID, lib
    from animal_vision_amd.runtime import get_context
    from animal_vision_amd.yuv import rgb_to_yuv, yuv_to_rgb

    ctx = get_context()
    d = ctx.malloc(4096)
    a, b = d.ptr, d.ptr + 2048
    try:
        # (fmt, yuv, rgb, n, H, W, matrix, full_range); the encode takes (rgb, yuv) in the other order
        bad = [(9, a, b, 1, 8, 8, 0, 0), (-1, a, b, 1, 8, 8, 0, 0), (1, a, a, 1, 8, 8, 0, 0), (1, a, a + 64, 1, 8, 8, 0, 0), (1, 0, b, 1, 8, 8, 0, 0),
               (1, a, 0, 1, 8, 8, 0, 0), (1, a, b, 0, 8, 8, 0, 0), (1, a, b, 1, 0, 8, 0, 0), (1, a, b, 1, 8, -8, 0, 0), (1, a, b, 1, 8, 8, 2, 0),
               (1, a, b, 1, 8, 8, 0, 2), (8, a + 1, b, 1, 8, 8, 0, 0)]
        for fmt, yuv, rgb, *rest in bad:
            for fn, args in ((lib.avx_yuv_to_rgb_u8, (fmt, yuv, rgb, *rest)), (lib.avx_rgb_to_yuv_u8, (fmt, rgb, yuv, *rest))):
                assert fn(ctx._h, *args, ctx.stream) == AVX_ERR_INVALID, (fn.__name__, args)
                assert lib.avx_last_error(ctx._h).decode().startswith(fn.__name__)
        assert lib.avx_yuv_to_rgb_u8(None, 1, a, b, 1, 8, 8, 0, 0, ctx.stream) == AVX_ERR_INVALID
    finally:
        d.free()
    with pytest.raises(ValueError):
        yuv_to_rgb(np.zeros(10, np.uint8), 4, 4, pix_fmt="nv12")
    with pytest.raises(ValueError):
        yuv_to_rgb(np.zeros(24, np.uint8), 4, 4, pix_fmt="nv21")
    with pytest.raises(ValueError):
        rgb_to_yuv(np.zeros((4, 4, 3), np.uint8), pix_fmt="p010le", matrix="bt2020")
    with pytest.raises(TypeError):
        yuv_to_rgb(np.zeros(24, np.uint16), 4, 4, pix_fmt="p010le")


# ---------------------------------------------------------------- FramePipeline(io_format="yuv") --------------------------------
def _run(pipe, frames):
    got = {}
    pipe.run(((i, f) for i, f in enumerate(frames)), lambda i, o: got.__setitem__(i, o))
    pipe.close()
    return [got[i] for i in range(len(frames))]


@pytest.mark.parametrize("fmt", ["nv12", "p010le"])
@pytest.mark.parametrize("species,H,W", [("dog", 96, 160), ("dog", 97, 161), ("reindeer", 96, 160), ("reindeer", 97, 161)])
def test_yuv_pipeline_equals_rgb_pipeline_through_the_encode(species, H, W, fmt):
    from animal_vision_amd.animals import Dog, Reindeer
    from animal_vision_amd.animals._uv_species import SpeciesStreamOp
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import FramePipeline

    yuv = R.encode(_frames(5, H, W, seed=11), fmt)
    rgb = list(R.decode(yuv, fmt, H, W))
    for split in (False, True):
        outs = {}
        for io in ("rgb", "yuv"):
            if species == "dog":
                op, close = DichromatOp(Dog.SPEC), None
            else:
                op = SpeciesStreamOp(Reindeer(), H, W, depth=3)
                close = op.close
            pipe = FramePipeline(op, H, W, depth=3, split_compare=split, io_format=io, pix_fmt=fmt if io == "yuv" else None)
            assert pipe.slots[0].h_in.array.nbytes == (H * W * 3 if io == "rgb" else R.frame_size(fmt, H, W))
            outs[io] = _run(pipe, rgb if io == "rgb" else list(yuv))
            if close:
                close()
        for k in range(len(rgb)):
            assert np.array_equal(outs["yuv"][k], R.encode(outs["rgb"][k], fmt)), (species, fmt, split, k)


def test_yuv_pipeline_batched_equals_unbatched():
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import FramePipeline

    H, W, fmt = 32, 48, "p010le"
    yuv = list(R.encode(_frames(5, H, W, seed=2), fmt))
    one = _run(FramePipeline(DichromatOp(Dog.SPEC), H, W, depth=2, io_format="yuv", pix_fmt=fmt), yuv)
    many = _run(FramePipeline(DichromatOp(Dog.SPEC), H, W, depth=2, io_format="yuv", pix_fmt=fmt, batch=2), yuv)
    assert all(np.array_equal(a, b) for a, b in zip(one, many))


# ---------------------------------------------------------------- run_video and the command ------------------------------------
def _write_raw(path, yuv):
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(yuv, np.uint8).tobytes())


@pytest.mark.parametrize("fmt", ["nv12", "yuv422p10le"])
def test_run_video_raw_world_1_and_2_byte_identical(tmp_path, oracle, fmt):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import run_video
    from animal_vision_amd.renderers import VideoRenderer

    H, W = 96, 160
    yuv = R.encode(_frames(7, H, W, seed=3), fmt)
    src = str(tmp_path / "in.yuv")
    _write_raw(src, yuv)
    for world in (1, 2):
        dst = str(tmp_path / f"out{world}.yuv")
        for rank in range(world):
            vr = VideoRenderer(read_path=src, write_path=dst, rank=rank, world=world, pix_fmt=fmt, size=(W, H))
            vr.open()
            assert vr.yuv_hw == (H, W) and vr.yuv_pix_fmt == fmt
            st = run_video(DichromatOp(Dog.SPEC), vr, rank=rank, world=world)
            vr.close()
            assert st.frames == len(range(rank, 7, world))
        if world > 1:
            vr.merge_shards()
    one = open(str(tmp_path / "out1.yuv"), "rb").read()
    assert one == open(str(tmp_path / "out2.yuv"), "rb").read()
    got = np.frombuffer(one, np.uint8).reshape(7, R.frame_size(fmt, H, W))
    for k in range(7):
        want = oracle.dichromat_visualize(oracle.DICHROMATS["dog"], R.decode(yuv[k], fmt, H, W))[1]
        assert np.array_equal(got[k], R.encode(want, fmt)), k


def test_raw_source_get_image_and_sinks_in_other_formats(tmp_path):
    """get_image() keeps its RGB contract on a raw source; a sink in another raw format and a .y4m sink go through RGB."""
    import _yuv_ref as R8
    from animal_vision_amd.renderers import VideoRenderer
    from animal_vision_amd.renderers.y4m import Y4MReader

    H, W, fmt = 97, 161, "p010le"
    yuv = R.encode(_frames(3, H, W, seed=5), fmt, "bt709", "full")
    src = str(tmp_path / "in.yuv")
    _write_raw(src, yuv)
    rgb = R.decode(yuv, fmt, H, W, "bt709", "full")
    for dst, wfmt in ((str(tmp_path / "o.yuv"), "yuv444p"), (str(tmp_path / "o.y4m"), None)):
        vr = VideoRenderer(read_path=src, write_path=dst, matrix="bt709", range="full", pix_fmt=fmt, size=(W, H), write_pix_fmt=wfmt)
        vr.open()
        assert vr.yuv_hw is None
        k = 0
        while (f := vr.get_image()) is not None:
            assert np.array_equal(f, rgb[k])
            vr.render(f)
            k += 1
        vr.close()
        assert k == 3
    assert open(str(tmp_path / "o.yuv"), "rb").read() == R.encode(rgb, "yuv444p", "bt709", "full").tobytes()
    rd = Y4MReader(str(tmp_path / "o.y4m"))
    assert rd.header.full_range and (rd.header.width, rd.header.height) == (W, H)
    for k in range(3):
        assert np.array_equal(rd.read(), R8.encode(rgb[k], "bt709", "full"))
    rd.close()


def test_cli_raw_nv12_file_and_stdin_to_stdout(tmp_path, capsys):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.renderers import split_compose
    from animal_vision_amd.video import main

    H, W, fmt = 64, 96, "nv12"
    yuv = R.encode(_frames(4, H, W, seed=9), fmt)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "dog.yuv")
    _write_raw(src, yuv)
    rgb = R.decode(yuv, fmt, H, W)
    args = ["--species", "Dog", "--split-compare", "--pix-fmt", fmt, "--size", f"{W}x{H}"]
    assert main([src, dst] + args) == 0
    assert "4 frames" in capsys.readouterr().err
    got = np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(4, -1)
    for k in range(4):
        want = split_compose(rgb[k], Dog().visualize(rgb[k])[1], left_label="Original", right_label="Transformed")
        assert np.array_equal(got[k], R.encode(want, fmt)), k
    # a different output format: through RGB on the way out
    dst10 = str(tmp_path / "dog10.yuv")
    assert main([src, dst10] + args + ["--out-pix-fmt", "p010le"]) == 0
    got10 = np.frombuffer(open(dst10, "rb").read(), np.uint8).reshape(4, -1)
    for k in range(4):
        want = split_compose(rgb[k], Dog().visualize(rgb[k])[1], left_label="Original", right_label="Transformed")
        assert np.array_equal(got10[k], R.encode(want, "p010le")), k
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "animal_vision_amd.video", "-", "-"] + args, input=open(src, "rb").read(), capture_output=True,
                         timeout=180, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    assert out.stdout == open(dst, "rb").read()
    assert b"4 frames" in out.stderr
