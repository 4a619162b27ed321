"""GPU: the frame-metrics kernel (csrc/metrics.hip) against the float64 definition of tests/_metrics_ref.py, and the
compare command end to end.  Small frames only: the sizes are where the tiling can go wrong (T = the kernel's 32 x 32 tile).

SSIM bound: 1e-5 absolute per frame and channel -- 15 x the worst case of a float32 emulation of the centred separable form over the
six frame pairs below (6.3e-7), and 7 x below what the uncentred float32 form does on flat 255 against flat 254 (6.7e-5), so a kernel
that forgets to centre fails."""
import ctypes
import math

import numpy as np
import pytest

import _metrics_ref as R
from animal_vision_amd import compare as _compare_module, metrics as _metrics_module  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu

T = 32
SIZES = [(10, 40), (40, 10), (11, 11), (11, 75), (75, 11), (37, 53), (T + 10, T + 10), (T + 11, T + 9), (270, 480)]
SSIM_TOL = 1e-5
_cache = {}


def _pairs(H, W):
    """The six frame pairs and one more of independent noise, with the reference's histogram and SSIM of each; computed once."""
    if (H, W) not in _cache:
        rng = np.random.default_rng(H * 1000 + W)
        pairs = R.six_frames(H, W, seed=H + W) + [("random", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))]
        a, b = np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs])
        a.setflags(write=False), b.setflags(write=False)
        _cache[(H, W)] = ([p[0] for p in pairs], a, b, [R.abs_hist(x, y) for x, y in zip(a, b)], [R.ssim(x, y) for x, y in zip(a, b)])
    return _cache[(H, W)]


def _same(m, n):
    return np.array_equal(m.abs_hist, n.abs_hist) and np.array(m.ssim).tobytes() == np.array(n.ssim).tobytes()


@pytest.mark.parametrize("H,W", SIZES)
def test_histogram_exact_and_ssim_within_bound(H, W):
    from animal_vision_amd.metrics import frame_metrics

    names, a, b, hists, ssims = _pairs(H, W)
    got = frame_metrics(a, b)
    worst = 0.0
    for name, m, h, s in zip(names, got, hists, ssims):
        assert np.array_equal(m.abs_hist, h), (name, H, W)
        assert m.sse == tuple(R.sse_from_hist(h)) and m.samples == H * W
        if H < 11 or W < 11:
            assert all(math.isnan(v) for v in m.ssim), (name, m.ssim)
        else:
            dev = max(abs(x - y) for x, y in zip(m.ssim, s))
            worst = max(worst, dev)
    print(f"metrics {H}x{W}: largest SSIM deviation {worst:.3e}")
    for name, m, s in zip(names, got, ssims):
        if H >= 11 and W >= 11:
            for c in range(3):
                assert abs(m.ssim[c] - s[c]) <= SSIM_TOL, (name, H, W, c, m.ssim[c], s[c])
    # with_ssim = 0: the same histograms, NaN
    for name, m, h in zip(names, frame_metrics(a, b, ssim=False), hists):
        assert np.array_equal(m.abs_hist, h) and all(math.isnan(v) for v in m.ssim), (name, H, W)


@pytest.mark.parametrize("H,W", [(11, 11), (37, 53), (T + 10, T + 10), (T + 11, T + 9), (270, 480), (10, 40)])
def test_identical_frames(H, W):
    from animal_vision_amd.metrics import frame_metrics

    _, a, _, _, _ = _pairs(H, W)
    for m in frame_metrics(a, a):
        assert [int(v) for v in m.abs_hist[:, 0]] == [H * W] * 3 and int(m.abs_hist.sum()) == 3 * H * W
        assert m.psnr == math.inf and m.psnr_channels == (math.inf,) * 3 and m.max_abs == 0
        if H >= 11 and W >= 11:
            assert m.ssim == (1.0, 1.0, 1.0)


def test_batches_are_bit_equal_to_single_frames_and_repeatable():
    from animal_vision_amd.metrics import frame_metrics

    H, W = 75, 107  # 3 x 4 tiles, nothing aligned
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (16, H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    b[3:] = rng.integers(0, 256, (13, H, W, 3), dtype=np.uint8)  # every frame pair different
    single = [frame_metrics(a[i], b[i]) for i in range(16)]
    assert len({np.array(m.ssim).tobytes() for m in single}) == 16
    for n in (1, 3, 16):
        got = frame_metrics(a[16 - n:], b[16 - n:])
        again = frame_metrics(a[16 - n:], b[16 - n:])
        assert len(got) == n
        for i in range(n):
            assert _same(got[i], single[16 - n + i]), (n, i)
            assert _same(got[i], again[i]), (n, i)
    more = frame_metrics(np.concatenate([a, a[:5]]), np.concatenate([b, b[:5]]))  # 21 frames: two chunks
    assert len(more) == 21 and all(_same(more[i], single[i % 16]) for i in range(21))


def test_bad_arguments_launch_nothing():
    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import RECORD_BYTES, frame_metrics
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 16, 16
    d_a, d_b = ctx.upload(np.zeros((H, W, 3), np.uint8)), ctx.upload(np.ones((H, W, 3), np.uint8))
    d_out = ctx.upload(np.full(RECORD_BYTES, 0xAB, np.uint8))
    fn = _lib.lib.avx_frame_metrics_u8
    try:
        for args in ((d_a.ptr, d_b.ptr, 0, H, W, d_out.ptr), (d_a.ptr, d_b.ptr, 17, H, W, d_out.ptr), (None, d_b.ptr, 1, H, W, d_out.ptr),
                     (d_a.ptr, None, 1, H, W, d_out.ptr), (d_a.ptr, d_b.ptr, 1, H, W, None), (d_a.ptr, d_b.ptr, 1, 0, W, d_out.ptr),
                     (d_a.ptr, d_b.ptr, 1, H, -3, d_out.ptr), (d_a.ptr, d_b.ptr, 1, 1 << 16, 1 << 16, d_out.ptr)):
            pa, pb, n, h, w, po = args
            rc = fn(ctx._h, pa, pb, n, h, w, 1, po, ctx.stream)
            assert rc == _lib.AVX_ERR_INVALID, args
            assert _lib.lib.avx_last_error(ctx._h).decode().startswith("avx_frame_metrics_u8:"), args
        ctx.sync()
        assert (ctx.download(d_out, (RECORD_BYTES,), np.uint8) == 0xAB).all()  # nothing was launched, nothing cleared
        assert fn(ctx._h, d_a.ptr, d_b.ptr, 1, H, W, 1, d_out.ptr, ctx.stream) == 0  # and the good call still works
        rec = np.frombuffer(ctx.download(d_out, (RECORD_BYTES,), np.uint8).tobytes(), np.uint32, count=768).reshape(3, 256)
        assert [int(v) for v in rec[:, 1]] == [H * W] * 3
    finally:
        for d in (d_a, d_b, d_out):
            d.free()
    with pytest.raises(ValueError, match=r"\(16, 16, 3\).*\(16, 17, 3\)"):
        frame_metrics(np.zeros((16, 16, 3), np.uint8), np.zeros((16, 17, 3), np.uint8))


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from animal_vision_amd.renderers import VideoRenderer

    d = tmp_path_factory.mktemp("metrics_clips")
    rng = np.random.default_rng(11)
    base = np.kron(rng.integers(0, 256, (12, 12, 16, 3), dtype=np.uint8), np.ones((1, 4, 4, 1), np.uint8))  # 48 x 64 blocks
    frames = np.clip(base.astype(np.int16) + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8)
    np.save(d / "twelve.npy", frames)
    np.save(d / "nine.npy", frames[:9])
    vr = VideoRenderer(read_path=None, write_path=str(d / "twelve.y4m"))
    vr.open()
    for f in frames:
        vr.render(f)
    vr.close()
    return d, frames


def _compare(capsys, argv):
    from animal_vision_amd import compare

    status = compare.main([str(v) for v in argv])
    cap = capsys.readouterr()
    return status, cap.out, cap.err


def test_command_npy_against_itself(clips, capsys):
    d, frames = clips
    status, out, err = _compare(capsys, [d / "twelve.npy", d / "twelve.npy"])
    lines = out.splitlines()
    assert status == 0 and len(lines) == 13
    for i, line in enumerate(lines[1:]):
        assert line == f"{i},inf,inf,inf,inf,1.000000,1.000000,1.000000,1.000000,0,0"
    assert "compare: 12 frames, PSNR inf dB" in err


def test_command_payload_route_equals_get_image_route(clips, capsys):
    from animal_vision_amd.compare import CSV_HEADER, format_row
    from animal_vision_amd.metrics import frame_metrics
    from animal_vision_amd.renderers import VideoRenderer

    d, frames = clips
    vr = VideoRenderer(read_path=str(d / "twelve.y4m"))
    vr.open()
    decoded = np.stack([vr.get_image() for _ in range(12)])
    assert vr.get_image() is None
    vr.close()
    assert not np.array_equal(decoded, frames)  # 4:2:0 is lossy: there is something to measure
    want = CSV_HEADER + "\n" + "".join(format_row(i, m) + "\n" for i, m in enumerate(frame_metrics(decoded, frames)))
    status, out5, err = _compare(capsys, [d / "twelve.y4m", d / "twelve.npy", "--batch", "5"])
    assert status == 0 and out5 == want
    status, out16, _ = _compare(capsys, [d / "twelve.y4m", d / "twelve.npy", "--batch", "16"])
    assert status == 0 and out16 == out5
    status, out8, _ = _compare(capsys, [d / "twelve.y4m", d / "twelve.y4m", "--no-ssim"])  # both sides payloads
    assert status == 0 and all(line.split(",")[1:5] == ["inf"] * 4 and line.split(",")[5:9] == ["nan"] * 4 for line in out8.splitlines()[1:])
    status, out, err = _compare(capsys, [d / "twelve.y4m", d / "twelve.npy", "--max-abs", "0"])
    assert status == 1 and "compare: frame 0:" in err and out == want


def test_command_lengths_and_sizes(clips, capsys, tmp_path):
    d, frames = clips
    status, out, err = _compare(capsys, [d / "nine.npy", d / "twelve.npy"])
    assert status == 2 and len(out.splitlines()) == 10 and "B has more frames" in err
    status, out, err = _compare(capsys, [d / "twelve.npy", d / "nine.npy", "--shortest", "--batch", "3"])  # the shorter one ends on a batch boundary
    assert status == 0 and len(out.splitlines()) == 10 and "more frames" not in err
    np.save(tmp_path / "small.npy", frames[:2, :40])
    with pytest.raises(SystemExit, match="frame sizes differ"):
        _compare(capsys, [d / "twelve.npy", tmp_path / "small.npy"])
    csv = tmp_path / "out.csv"
    status, out, err = _compare(capsys, [d / "twelve.npy", d / "twelve.y4m", "--scale", "32x24", "--csv", csv])  # scaled: both through get_image
    assert status == 0 and out == "" and len(csv.read_text().splitlines()) == 13
