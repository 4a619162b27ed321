"""CPU: the raw pixel format arithmetic of DESIGN §4.9 -- the C side's coefficient tables against the NumPy restatement
(tests/_rawyuv_ref.py), the restatement against the float64 formula at 10 bits, frame sizes, the raw reader / writer, the
`video` command's new flags and FramePipeline's argument checks.  No device is used."""
import ctypes
import os
import threading

import numpy as np
import pytest

import _rawyuv_ref as R
import _yuv_ref as R8

SIZES = [(1, 1), (3, 18), (97, 161), (1080, 1920)]


# ---------------------------------------------------------------- coefficient tables ------------------------------------------
@pytest.mark.parametrize("matrix,rng", R.COMBOS)
@pytest.mark.parametrize("d", [8, 10])
def test_c_tables_equal_the_restatement(matrix, rng, d):
    from animal_vision_amd.yuv import coefficients

    dec, enc = coefficients(matrix, rng, depth=d)
    assert dec == R.dec_coef(matrix, rng, d)
    assert enc == R.enc_coef(matrix, rng, d)


@pytest.mark.parametrize("matrix,rng", R.COMBOS)
def test_depth_8_tables_are_the_i420_tables(matrix, rng):
    from animal_vision_amd._lib import lib
    from animal_vision_amd.yuv import MATRICES, RANGES, coefficients

    assert coefficients(matrix, rng, depth=8) == coefficients(matrix, rng)
    a = ((ctypes.c_int * 6)(), (ctypes.c_int * 10)())
    b = ((ctypes.c_int * 6)(), (ctypes.c_int * 10)())
    assert lib.avx_yuv_coefficients(MATRICES[matrix], RANGES[rng], *a) == 0
    assert lib.avx_yuv_coefficients_d(MATRICES[matrix], RANGES[rng], 8, *b) == 0
    assert list(a[0]) == list(b[0]) and list(a[1]) == list(b[1])
    assert R.dec_coef(matrix, rng, 8) == R8.dec_coef(matrix, rng) and R.enc_coef(matrix, rng, 8) == R8.enc_coef(matrix, rng)


def test_coefficients_d_refuses_bad_arguments():
    from animal_vision_amd._lib import AVX_ERR_INVALID, lib

    d, e = (ctypes.c_int * 6)(), (ctypes.c_int * 10)()
    for args in ((2, 0, 8), (0, 2, 8), (0, 0, 9), (0, 0, 12), (0, 0, 16), (-1, 0, 10)):
        assert lib.avx_yuv_coefficients_d(*args, d, e) == AVX_ERR_INVALID, args
    assert lib.avx_yuv_coefficients_d(0, 0, 10, None, e) == AVX_ERR_INVALID
    assert lib.avx_yuv_coefficients_d(0, 0, 10, d, None) == AVX_ERR_INVALID
    with pytest.raises(ValueError):
        from animal_vision_amd.yuv import coefficients

        coefficients("bt601", "limited", depth=12)


@pytest.mark.parametrize("matrix,rng", R.COMBOS)
@pytest.mark.parametrize("d", [8, 10])
def test_encode_rows_sum_exactly_and_greys_are_neutral(matrix, rng, d):
    (ry, ru, rv), yo = R.enc_coef(matrix, rng, d)
    _, ys, _ = R.range_params(rng, d)
    assert sum(ry) == R.q16(ys) and sum(ru) == 0 and sum(rv) == 0
    fmt = "yuv444p" if d == 8 else "yuv444p10le"
    grey = np.repeat(np.arange(256, dtype=np.uint8), 3).reshape(1, 256, 3)
    _, U, V = R.split_planes(R.encode(grey, fmt, matrix, rng), fmt, 1, 256)
    assert (U == 1 << (d - 1)).all() and (V == 1 << (d - 1)).all()
    for f in ("yuv420p10le", "p010le", "yuv422p10le", "nv12"):  # block sums of 2 and 4 equal greys
        g2 = np.broadcast_to(grey, (2, 256, 3))
        _, U, V = R.split_planes(R.encode(g2, f, matrix, rng), f, 2, 256)
        assert (U == 1 << (R.depth_of(f) - 1)).all() and (V == 1 << (R.depth_of(f) - 1)).all(), f


# ---------------------------------------------------------------- 10-bit fixed point against float64 ---------------------------
def _triples_10bit():
    """An 11^3 lattice of extremes plus 4 M random (Y, U, V) triples of 10-bit samples."""
    ax = np.array([0, 1, 63, 64, 511, 512, 513, 939, 940, 1022, 1023])
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rnd = np.random.default_rng(10).integers(0, 1024, (4_000_000, 3))
    return np.concatenate([lat, rnd])


@pytest.mark.parametrize("matrix,rng", R.COMBOS)
def test_10bit_decode_within_one_code_of_float64(matrix, rng):
    t = _triples_10bit()
    got = np.stack(R.decode_px(t[:, 0], t[:, 1], t[:, 2], matrix, rng, 10), -1).astype(np.float64)
    want = np.clip(np.stack(R.decode_float(t[:, 0], t[:, 1], t[:, 2], matrix, rng, 10), -1), 0, 255)
    assert np.abs(got - want).max() <= 1.0
    # the accumulator stays inside int32 (the device computes it in int32)
    cy, crv, cgu, cgv, cbu, yo = R.dec_coef(matrix, rng, 10)
    worst = abs(cy) * 1023 + max(abs(crv), abs(cgu) + abs(cgv), abs(cbu)) * 512 + (1 << 15)
    assert worst < 2 ** 31


@pytest.mark.parametrize("matrix,rng", R.COMBOS)
def test_10bit_encode_within_one_code_of_float64(matrix, rng):
    ax = np.array([0, 1, 2, 16, 127, 128, 129, 235, 253, 254, 255])
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rgb = np.concatenate([lat, np.random.default_rng(11).integers(0, 256, (1_000_000, 3))]).astype(np.uint8)
    pay = R.encode(rgb.reshape(1, 1, -1, 3), "yuv444p10le", matrix, rng)
    Y, U, V = (p.reshape(-1).astype(np.float64) for p in R.split_planes(pay, "yuv444p10le", 1, len(rgb)))
    fy, fu, fv = (np.clip(x, 0, 1023) for x in R.encode_float(rgb[:, 0], rgb[:, 1], rgb[:, 2], matrix, rng, 10))
    assert max(np.abs(Y - fy).max(), np.abs(U - fu).max(), np.abs(V - fv).max()) <= 1.0
    (ry, ru, rv), _ = R.enc_coef(matrix, rng, 10)
    assert max(sum(abs(c) for c in row) for row in (ry, ru, rv)) * 4 * 255 + (1 << 17) < 2 ** 31


def test_restatement_at_8_bits_equals_the_i420_restatement():
    rgb = np.random.default_rng(3).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    for matrix, rng in R.COMBOS:
        assert np.array_equal(R.encode(rgb, "yuv420p", matrix, rng), R8.encode(rgb, matrix, rng))
        pay = R.random_payload("yuv420p", 2, 5, 7, 4)
        assert np.array_equal(R.decode(pay, "yuv420p", 5, 7, matrix, rng), R8.decode(pay, 5, 7, matrix, rng))


def test_p010_and_nv12_are_the_planar_forms_rearranged():
    rgb = np.random.default_rng(5).integers(0, 256, (2, 6, 10, 3), dtype=np.uint8)
    for il, pl in (("nv12", "yuv420p"), ("p010le", "yuv420p10le")):
        a, b = R.split_planes(R.encode(rgb, il), il, 6, 10), R.split_planes(R.encode(rgb, pl), pl, 6, 10)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    p = R.encode(rgb, "p010le")
    assert (p[:, 0::2] & 63 == 0).all()


# ---------------------------------------------------------------- frame sizes --------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_frame_size_every_format(H, W):
    from animal_vision_amd.yuv import PIX_FMTS, frame_size, i420_size

    assert set(PIX_FMTS) == set(R.FORMATS)
    cw, ch = (W + 1) // 2, (H + 1) // 2
    want = {"yuv420p": H * W + 2 * ch * cw, "nv12": H * W + 2 * ch * cw, "yuv422p": H * W + 2 * H * cw, "yuv444p": 3 * H * W, "gray": H * W,
            "yuv420p10le": 2 * (H * W + 2 * ch * cw), "yuv422p10le": 2 * (H * W + 2 * H * cw), "yuv444p10le": 6 * H * W,
            "p010le": 2 * (H * W + 2 * ch * cw)}
    for f in PIX_FMTS:
        assert frame_size(f, H, W) == want[f] == R.frame_size(f, H, W), f
    assert frame_size("yuv420p", H, W) == i420_size(H, W)


def test_frame_size_refuses_bad_arguments():
    from animal_vision_amd._lib import lib
    from animal_vision_amd.yuv import frame_size

    assert lib.avx_yuv_frame_size(9, 4, 4) == 0 and lib.avx_yuv_frame_size(-1, 4, 4) == 0 and lib.avx_yuv_frame_size(0, 0, 4) == 0
    with pytest.raises(ValueError):
        frame_size("yuv420p12le", 4, 4)
    with pytest.raises(ValueError):
        frame_size("nv12", 0, 4)


# ---------------------------------------------------------------- raw reader and writer ----------------------------------------
def _write_raw(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            f.write(np.asarray(fr, np.uint8).tobytes())


def test_raw_reader_sharded_indexing_and_round_trip(tmp_path):
    from animal_vision_amd.renderers.rawvideo import RawVideoReader, RawVideoWriter

    H, W, fmt = 6, 10, "p010le"
    frames = R.random_payload(fmt, 7, H, W, 1)
    src = str(tmp_path / "in.yuv")
    _write_raw(src, frames)
    for world in (1, 2, 3):
        seen = {}
        for rank in range(world):
            rd = RawVideoReader(src, fmt, W, H, rank=rank, world=world)
            assert rd.total_frames == 7 and rd.frame_size == R.frame_size(fmt, H, W)
            while (f := rd.read()) is not None:
                assert rd.last_index % world == rank
                seen[rd.last_index] = f
            assert rd.read() is None
            rd.close()
        assert sorted(seen) == list(range(7))
        assert all(np.array_equal(seen[k], frames[k]) for k in range(7))
    dst = str(tmp_path / "out.yuv")
    rd, wr = RawVideoReader(src, fmt, W, H), RawVideoWriter(dst, fmt, W, H)
    while (f := rd.read()) is not None:
        wr.write(f)
    rd.close()
    wr.close()
    assert wr.frames == 7 and open(dst, "rb").read() == open(src, "rb").read()
    with pytest.raises(ValueError):
        RawVideoWriter(str(tmp_path / "x.yuv"), fmt, W, H).write(np.zeros(5, np.uint8))


def test_raw_reader_refuses_a_partial_file_bad_ranks_and_bad_formats(tmp_path):
    from animal_vision_amd.renderers.rawvideo import RawVideoReader

    H, W = 4, 6
    src = str(tmp_path / "in.yuv")
    with open(src, "wb") as f:
        f.write(bytes(R.frame_size("nv12", H, W) * 2 + 5))
    with pytest.raises(ValueError, match="whole number"):
        RawVideoReader(src, "nv12", W, H)
    with pytest.raises(ValueError):
        RawVideoReader(src, "nv12", W, H, rank=2, world=2)
    with pytest.raises(ValueError):
        RawVideoReader(src, "yuv411p", W, H)
    with pytest.raises(ValueError):
        RawVideoReader(src, "nv12", 0, H)


def _feed(path, data):
    def run():
        with open(path, "wb") as f:
            f.write(data)

    t = threading.Thread(target=run)
    t.start()
    return t


def test_raw_reader_fifo_is_sequential_one_rank_and_names_a_truncated_frame(tmp_path):
    from animal_vision_amd.renderers.rawvideo import RawVideoReader

    H, W, fmt = 4, 6, "nv12"
    frames = R.random_payload(fmt, 3, H, W, 2)
    fifo = str(tmp_path / "pipe")
    os.mkfifo(fifo)
    with pytest.raises(ValueError, match="world"):
        RawVideoReader(fifo, fmt, W, H, rank=0, world=2)
    t = _feed(fifo, frames.tobytes() + b"\x00" * 7)
    rd = RawVideoReader(fifo, fmt, W, H)
    assert rd.sequential and rd.total_frames is None
    for k in range(3):
        assert np.array_equal(rd.read(), frames[k]) and rd.last_index == k
    with pytest.raises(ValueError, match="frame 3 is truncated"):
        rd.read()
    rd.close()
    t.join()
    t = _feed(fifo, frames[:2].tobytes())  # a stream that ends on a frame boundary ends cleanly
    rd = RawVideoReader(fifo, fmt, W, H)
    assert rd.read() is not None and rd.read() is not None and rd.read() is None
    rd.close()
    t.join()


def test_video_renderer_raw_arguments(tmp_path):
    from animal_vision_amd.renderers import VideoRenderer

    H, W, fmt = 4, 6, "nv12"
    frames = R.random_payload(fmt, 5, H, W, 3)
    src = str(tmp_path / "in.yuv")
    _write_raw(src, frames)
    with pytest.raises(ValueError):
        VideoRenderer(read_path=src, pix_fmt=fmt)                       # no size
    with pytest.raises(ValueError):
        VideoRenderer(read_path=src, size=(W, H))                       # no format
    with pytest.raises(ValueError):
        VideoRenderer(read_path=src, pix_fmt="yuv411p", size=(W, H))
    with pytest.raises(ValueError):
        VideoRenderer(read_path=src, write_path="-", pix_fmt=fmt, size=(W, H), world=2)
    # same format in and out: payloads stay payloads; world 2 shards merge into the world 1 bytes
    for world in (1, 2):
        dst = str(tmp_path / f"out{world}.yuv")
        for rank in range(world):
            vr = VideoRenderer(read_path=src, write_path=dst, pix_fmt=fmt, size=(W, H), rank=rank, world=world)
            vr.open()
            assert vr.write_pix_fmt == fmt and vr.yuv_hw == (H, W) and vr.yuv_pix_fmt == fmt and vr.total_frames == 5
            while (f := vr.get_yuv()) is not None:
                vr.render(f, index=vr.last_index)
            vr.close()
        if world > 1:
            assert vr.merge_shards() == dst
            assert not os.path.exists(str(tmp_path / "out2.rank0of2.yuv"))
        assert open(dst, "rb").read() == open(src, "rb").read()
    # other sinks: through RGB
    assert VideoRenderer(read_path=src, write_path=str(tmp_path / "o.y4m"), pix_fmt=fmt, size=(W, H)).write_pix_fmt is None
    vr = VideoRenderer(read_path=src, write_path=str(tmp_path / "o.y4m"), pix_fmt=fmt, size=(W, H))
    vr.open()
    assert vr.yuv_hw is None
    vr.close()
    vr = VideoRenderer(read_path=src, write_path=str(tmp_path / "o2.yuv"), pix_fmt=fmt, size=(W, H), write_pix_fmt="p010le")
    vr.open()
    assert vr.yuv_hw is None and vr.write_pix_fmt == "p010le"
    vr.close()
    # without the new arguments nothing changes
    vr = VideoRenderer(read_path="synthetic:8x8:2", write_path=str(tmp_path / "o.npy"))
    assert vr.pix_fmt is None and vr.write_pix_fmt is None and vr.size is None


# ---------------------------------------------------------------- the command's flags and the pipeline's checks ---------------
def test_cli_flags():
    from animal_vision_amd.video import parse_args

    a = parse_args(["-", "out.yuv", "--species", "Dog", "--pix-fmt", "p010le", "--size", "3840x2160"])
    assert a.pix_fmt == "p010le" and a.size == (3840, 2160) and a.out_pix_fmt is None
    a = parse_args(["in.yuv", "out.yuv", "--species", "Dog", "--pix-fmt", "nv12", "--size", "64X48", "--out-pix-fmt", "yuv444p10le"])
    assert a.size == (64, 48) and a.out_pix_fmt == "yuv444p10le"
    a = parse_args(["in.y4m", "out.y4m", "--species", "Dog"])
    assert a.pix_fmt is None and a.size is None and a.out_pix_fmt is None and a.batch == 1 and a.depth == 3 and a.matrix == "bt601"
    for bad in (["--pix-fmt", "nv12"], ["--size", "64x48"], ["--pix-fmt", "nv12", "--size", "64"], ["--pix-fmt", "nv12", "--size", "0x4"],
                ["--pix-fmt", "nv21", "--size", "64x48"], ["--out-pix-fmt", "yuv420p12le"]):
        with pytest.raises(SystemExit):
            parse_args(["in.yuv", "out.yuv", "--species", "Dog"] + bad)


def test_pipeline_refuses_yuv_without_a_format_before_it_touches_the_device():
    from animal_vision_amd.pipeline import FramePipeline

    class Op:  # never reached: the checks come before any allocation
        ctx = None

    with pytest.raises(ValueError, match="pix_fmt"):
        FramePipeline(Op(), 16, 16, io_format="yuv")
    with pytest.raises(ValueError, match="pix_fmt"):
        FramePipeline(Op(), 16, 16, io_format="yuv", pix_fmt="nv21")
    with pytest.raises(ValueError, match="pix_fmt"):
        FramePipeline(Op(), 16, 16, io_format="i420", pix_fmt="nv12")
    with pytest.raises(ValueError, match="io_format"):
        FramePipeline(Op(), 16, 16, io_format="nv12")
