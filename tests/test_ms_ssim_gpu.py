"""GPU: MS-SSIM over five scales (csrc/ms_ssim.hip) against the float64 definition of tests/_ms_ssim_ref.py, and
compare --ms-ssim end to end.  The sizes are where the pyramid and the tilings can go wrong: 176 (one window position at scale 4), odd
sizes whose frames put every later frame of a batch on an odd address, sizes off the pyramid's 32 x 32 source tile and off the 32 x 32
tile of window positions, and one 1080p pair (scales of 540, 270, 135, 67 rows: an odd drop in the middle, many tiles).

Bound: 1e-5 absolute on every per-scale mean, the project's SSIM bound (tests/test_metrics_gpu.py) taken over unchanged.  Scale 0 is
that kernel's float32 arithmetic; scales 1..4 are float64 on exact samples and land many orders below it."""
import numpy as np
import pytest

import _metrics_ref as R
import _ms_ssim_ref as M
from animal_vision_amd import compare as _compare_module, metrics as _metrics_module  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-5
_cache = {}


def _six(H, W):
    """The six frame pairs at H x W with the reference's per-scale means; computed once."""
    if (H, W) not in _cache:
        pairs = R.six_frames(H, W, seed=H + W)
        a, b = np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs])
        a.setflags(write=False), b.setflags(write=False)
        _cache[(H, W)] = ([p[0] for p in pairs], a, b, [M.levels(x, y) for x, y in zip(a, b)])
    return _cache[(H, W)]


def _noise_pair(H, W, k, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-k, k + 1, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _check(name, H, W, got, want):
    """One frame's record against the reference's (cs, ssim); the largest deviation."""
    cs, ss = want
    dev = max(float(np.abs(got.cs - cs).max()), float(np.abs(got.ssim - ss).max()))
    for c in range(3):
        for j in range(5):
            assert abs(got.cs[c][j] - cs[c][j]) <= TOL, (name, H, W, "cs", c, j, got.cs[c][j], cs[c][j])
            assert abs(got.ssim[c][j] - ss[c][j]) <= TOL, (name, H, W, "ssim", c, j, got.ssim[c][j], ss[c][j])
        # the product is formed on the host from the device's own means
        want_c = M.combine(got.cs[c], got.ssim[c])
        assert abs(got.ms_ssim_channels[c] - want_c) <= 1e-12 * max(want_c, 1e-300), (name, H, W, c)
    assert abs(got.ms_ssim - float(np.mean([M.combine(got.cs[c], got.ssim[c]) for c in range(3)]))) <= 1e-12
    return dev


@pytest.mark.parametrize("H,W", [(176, 176), (177, 207)])
def test_six_pairs_within_bound(H, W):
    from animal_vision_amd.metrics import ms_ssim

    names, a, b, refs = _six(H, W)
    got = ms_ssim(a, b)  # one batch of six: at 177 x 207 a frame is 109,917 bytes, every second frame starts on an odd address
    worst, worst0 = 0.0, 0.0
    for name, m, ref in zip(names, got, refs):
        worst = max(worst, float(np.abs(m.cs[:, 1:] - ref[0][:, 1:]).max()), float(np.abs(m.ssim[:, 1:] - ref[1][:, 1:]).max()))
        worst0 = max(worst0, float(np.abs(m.cs[:, 0] - ref[0][:, 0]).max()), float(np.abs(m.ssim[:, 0] - ref[1][:, 0]).max()))
    print(f"ms_ssim {H}x{W}: largest per-scale deviation {worst0:.3e} at scale 0, {worst:.3e} at scales 1..4")
    for name, m, ref in zip(names, got, refs):
        _check(name, H, W, m, ref)
    inv = got[names.index("inverse")]
    assert (inv.cs[:, :3] < 0).all() and inv.ms_ssim_channels == (0.0, 0.0, 0.0) and inv.ms_ssim == 0.0  # negative means kept, product 0
    # and a single frame through the array form gives one object, equal to its record in the batch
    one = ms_ssim(a[1], b[1])
    assert one == got[1]


@pytest.mark.parametrize("H,W", [(191, 176), (192, 208), (200, 263)])
def test_shapes(H, W):
    from animal_vision_amd.metrics import ms_ssim

    pairs = R.six_frames(H, W, seed=H * W)
    sel = [p for p in pairs if p[0] in ("ramp_noise8", "independent")] + [("noise_pm3",) + _noise_pair(H, W, 3, H)]
    got = ms_ssim(np.stack([p[1] for p in sel]), np.stack([p[2] for p in sel]))
    worst = max(_check(p[0], H, W, m, M.levels(p[1], p[2])) for p, m in zip(sel, got))
    print(f"ms_ssim {H}x{W}: largest per-scale deviation {worst:.3e}")
    same = ms_ssim(sel[0][2], sel[0][2])
    assert (same.cs == 1.0).all() and (same.ssim == 1.0).all() and same.ms_ssim == 1.0  # identical frames: exactly 1 at every scale


def test_1080p_noise_pm3():
    from animal_vision_amd.metrics import ms_ssim

    H, W = 1080, 1920
    a, b = _noise_pair(H, W, 3, 1080)
    got = ms_ssim(a, b)
    dev = _check("noise_pm3", H, W, got, M.levels(a, b))
    print(f"ms_ssim {H}x{W}: largest per-scale deviation {dev:.3e}, ms_ssim {got.ms_ssim:.9f}")


def test_base_record_is_byte_identical_and_scale0_bit_equal():
    from animal_vision_amd.metrics import (MS_RECORD_BYTES, RECORD_BYTES, frame_metrics_launch, frame_metrics_ms_launch, ms_records_from_bytes,
                                           records_from_bytes)
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    for H, W in ((177, 207), (192, 208)):
        pairs = R.six_frames(H, W, seed=1)
        a, b = np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs])
        n = len(a)
        d_a, d_b = ctx.upload(np.ascontiguousarray(a)), ctx.upload(np.ascontiguousarray(b))
        d_base, d_out = ctx.upload(np.full(n * RECORD_BYTES, 0xAB, np.uint8)), ctx.upload(np.full(n * RECORD_BYTES, 0xCD, np.uint8))
        d_ms = ctx.upload(np.full(n * MS_RECORD_BYTES, 0xEF, np.uint8))
        try:
            frame_metrics_launch(ctx, d_a, d_b, n, H, W, d_base, ssim=True)
            frame_metrics_ms_launch(ctx, d_a, d_b, n, H, W, d_out, d_ms)
            base = ctx.download(d_base, (n * RECORD_BYTES,), np.uint8)
            out = ctx.download(d_out, (n * RECORD_BYTES,), np.uint8)
            ms = ms_records_from_bytes(ctx.download(d_ms, (n * MS_RECORD_BYTES,), np.uint8), n)
        finally:
            for d in (d_a, d_b, d_base, d_out, d_ms):
                d.free()
        assert base.tobytes() == out.tobytes(), (H, W)
        for m, r in zip(records_from_bytes(base, n), ms):
            assert np.array(m.ssim).tobytes() == np.ascontiguousarray(r.ssim[:, 0]).tobytes(), (H, W)
            assert np.isfinite(r.cs).all() and np.isfinite(r.ssim).all()  # every field of the record was written


def test_batches_are_bit_equal_to_single_frames_and_repeatable():
    from animal_vision_amd.metrics import ms_ssim

    H, W = 177, 207
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (16, H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    b[3:] = rng.integers(0, 256, (13, H, W, 3), dtype=np.uint8)
    alone = ms_ssim(a[0], b[0])
    first, again = ms_ssim(a, b), ms_ssim(a, b)
    assert len(first) == 16 and first[0] == alone
    assert all(x == y for x, y in zip(first, again))  # from run to run
    order = [15] + list(range(1, 15)) + [0]           # the same pair at position 15, among the other pairs
    moved = ms_ssim(a[order], b[order])
    assert moved[15] == alone and moved[0] == first[15]
    assert len({m.cs.tobytes() + m.ssim.tobytes() for m in first}) == 16
    more = ms_ssim(np.concatenate([a, a[:3]]), np.concatenate([b, b[:3]]))  # 19 frames: two chunks
    assert len(more) == 19 and all(more[i] == first[i % 16] for i in range(19))


def test_bad_arguments_launch_nothing():
    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import MS_RECORD_BYTES, RECORD_BYTES, frame_metrics_ms_device, ms_records_from_bytes, ms_ssim
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 176, 176
    a, b = _noise_pair(H, W, 2, 9)
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    d_out, d_ms = ctx.upload(np.full(RECORD_BYTES, 0xAB, np.uint8)), ctx.upload(np.full(MS_RECORD_BYTES, 0xAB, np.uint8))
    fn = _lib.lib.avx_frame_metrics_ms_u8
    try:
        good, = frame_metrics_ms_device(ctx, d_a, d_b, 1, H, W)[1]
        ctx.upload(np.full(MS_RECORD_BYTES, 0xAB, np.uint8), d_ms)
        for args in ((d_a.ptr, d_b.ptr, 1, 175, W, d_out.ptr, d_ms.ptr), (d_a.ptr, d_b.ptr, 1, H, 175, d_out.ptr, d_ms.ptr),
                     (d_a.ptr, d_b.ptr, 0, H, W, d_out.ptr, d_ms.ptr), (d_a.ptr, d_b.ptr, 17, H, W, d_out.ptr, d_ms.ptr),
                     (None, d_b.ptr, 1, H, W, d_out.ptr, d_ms.ptr), (d_a.ptr, None, 1, H, W, d_out.ptr, d_ms.ptr),
                     (d_a.ptr, d_b.ptr, 1, H, W, None, d_ms.ptr), (d_a.ptr, d_b.ptr, 1, H, W, d_out.ptr, None)):
            pa, pb, n, h, w, po, pm = args
            assert fn(ctx._h, pa, pb, n, h, w, po, pm, ctx.stream) == _lib.AVX_ERR_INVALID, args
            msg = _lib.lib.avx_last_error(ctx._h).decode()
            assert msg.startswith("avx_frame_metrics_ms_u8:"), (args, msg)
            if h < 176 or w < 176:
                assert "176" in msg, msg
            ctx.sync()
            assert (ctx.download(d_out, (RECORD_BYTES,), np.uint8) == 0xAB).all() and (ctx.download(d_ms, (MS_RECORD_BYTES,), np.uint8) == 0xAB).all()
            assert fn(ctx._h, d_a.ptr, d_b.ptr, 1, H, W, d_out.ptr, d_ms.ptr, ctx.stream) == 0  # a correct call still works after each
            assert ms_records_from_bytes(ctx.download(d_ms, (MS_RECORD_BYTES,), np.uint8), 1)[0] == good
            ctx.upload(np.full(RECORD_BYTES, 0xAB, np.uint8), d_out)
            ctx.upload(np.full(MS_RECORD_BYTES, 0xAB, np.uint8), d_ms)
    finally:
        for d in (d_a, d_b, d_out, d_ms):
            d.free()
    for shape in ((175, 176, 3), (176, 175, 3)):
        with pytest.raises(ValueError, match="176"):
            ms_ssim(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8))
    assert ms_ssim(a, b) == good


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("ms_ssim_clips")
    rng = np.random.default_rng(21)
    base = np.kron(rng.integers(0, 256, (3, 11, 13, 3), dtype=np.uint8), np.ones((1, 16, 16, 1), np.uint8))  # 176 x 208, 16 x 16 blocks
    a = np.clip(base.astype(np.int16) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8)
    b = a.copy()
    b[1] = np.clip(a[1].astype(np.int16) + rng.integers(-60, 61, a[1].shape), 0, 255).astype(np.uint8)  # frame 1: far worse than 0 and 2
    b[0] = np.clip(a[0].astype(np.int16) + rng.integers(-2, 3, a[0].shape), 0, 255).astype(np.uint8)
    b[2] = np.clip(a[2].astype(np.int16) + rng.integers(-2, 3, a[2].shape), 0, 255).astype(np.uint8)
    np.save(d / "a.npy", a)
    np.save(d / "b.npy", b)
    return d, a, b


def _compare(capsys, argv):
    from animal_vision_amd import compare

    status = compare.main([str(v) for v in argv])
    cap = capsys.readouterr()
    return status, cap.out, cap.err


def test_command_ms_ssim(clips, capsys, tmp_path):
    from animal_vision_amd.compare import CSV_HEADER, CSV_MS_COLUMNS
    from animal_vision_amd.pairs import num as _num
    from animal_vision_amd.metrics import ms_ssim

    d, a, b = clips
    want = ms_ssim(a, b)
    status, plain, _ = _compare(capsys, [d / "a.npy", d / "b.npy"])
    assert status == 0 and plain.splitlines()[0] == CSV_HEADER
    csv = tmp_path / "q.csv"
    status, out, err = _compare(capsys, [d / "a.npy", d / "b.npy", "--ms-ssim", "--csv", csv])
    lines = csv.read_text().splitlines()
    assert status == 0 and out == "" and lines[0] == CSV_HEADER + CSV_MS_COLUMNS and len(lines) == 4
    assert [line.rsplit(",", 4)[0] for line in lines] == plain.splitlines()  # the other columns: the run without the flag
    for line, m in zip(lines[1:], want):
        assert line.split(",")[-4:] == [_num(v) for v in m.ms_ssim_channels] + [_num(m.ms_ssim)]
    vals = [m.ms_ssim for m in want]
    assert f"MS-SSIM mean {sum(vals) / 3:.6f} min {min(vals):.6f}" in err
    # a threshold between the clips' values: frame 1 is named, every line is still written
    assert vals[1] < min(vals[0], vals[2]) - 0.01
    thr = (vals[1] + min(vals[0], vals[2])) / 2
    status, out, err = _compare(capsys, [d / "a.npy", d / "b.npy", "--min-ms-ssim", f"{thr:.6f}", "--batch", "2"])
    assert status == 1 and "compare: frame 1: MS-SSIM" in err and out.splitlines() == lines
    status, out, err = _compare(capsys, [d / "a.npy", d / "a.npy", "--min-ms-ssim", "1"])
    assert status == 0 and all(line.split(",")[-4:] == ["1.000000"] * 4 for line in out.splitlines()[1:]) and "MS-SSIM mean 1.000000 min 1.000000" in err
