"""GPU: the difference-map kernels (csrc/diff_map.hip) against the definitions of tests/_diff_ref.py, and the diff command
end to end.  Small frames only: the sizes are where the vector path, the tiling (T = the SSIM kernel's 32 x 32 tile) and the replicated
5-pixel border can go wrong.

abs and heat maps and every record are integers: byte-equal to the reference.  The SSIM of a position is float32 on the device: each is
held to tol = 4 x max |map32 - float64 map| over the test's own frames, where map32 (tests/_diff_ref.py) restates the float32
arithmetic of csrc/ssim_window.h operation for operation on the CPU -- the bound is the error that form has by construction, times 4,
and never comes from the device.  The per-frame bound of the record (1e-5) does not carry over to positions: low-variance regions are
the hard case.  The mean of the returned float32 positions, summed in float64, equals the record of frame_metrics within 1e-9: the same
float32 numbers in another order of a float64 sum differ by n * 2^-53 relative at most; a map kernel with arithmetic of its own fails it."""
import numpy as np
import pytest

import _diff_ref as D
import _metrics_ref as R
from animal_vision_amd import diff as _diff_module  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu

T = 32
SIZES = [(1, 1), (3, 5), (2, 16), (32, 64), (11, 11), (11, 75), (75, 11), (37, 53), (T + 10, T + 10), (T + 11, T + 9), (75, 107)]
SSIM_SIZES = [s for s in SIZES if s[0] >= 11 and s[1] >= 11]
_cache = {}


def _pairs(H, W):
    """The six frame pairs, one of independent noise and the planted pair; computed once, read-only."""
    if (H, W) not in _cache:
        rng = np.random.default_rng(H * 1000 + W)
        pairs = R.six_frames(H, W, seed=H + W) + [("random", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))]
        if H >= 3 and W >= 3:
            pairs.append(("planted",) + D.planted_pair(H, W, (H - 3) // 2, (W - 3) // 3))
        a, b = np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs])
        a.setflags(write=False), b.setflags(write=False)
        _cache[(H, W)] = ([p[0] for p in pairs], a, b)
    return _cache[(H, W)]


_ssim_cache = {}


def _ssim_ref(H, W):
    """Per pair of _pairs(H, W): the float64 SSIM of every position, and tol = 4 x the largest deviation of map32 from it."""
    if (H, W) not in _ssim_cache:
        _, a, b = _pairs(H, W)
        pos = np.stack([D.ssim_positions(x, y) for x, y in zip(a, b)])
        m32 = np.stack([D.map32(x, y) for x, y in zip(a, b)])
        tol = 4.0 * float(np.abs(m32.astype(np.float64) - pos).max())
        pos.setflags(write=False)
        _ssim_cache[(H, W)] = (pos, tol)
    return _ssim_cache[(H, W)]


def _ref(mode, a, b, G, K, layout):
    m = D.abs_map(a, b, G) if mode == "abs" else D.heat_map(a, b, G, K)
    return D.side(a, b, m) if layout == "side" else m


# ------------------------------------------------------------------------------------------------ abs and heat
@pytest.mark.parametrize("H,W", SIZES)
def test_abs_and_heat_are_byte_equal_to_the_definition(H, W):
    from animal_vision_amd.metrics import diff_map

    names, a, b = _pairs(H, W)
    for mode in ("abs", "heat"):
        for layout in ("map", "side"):
            for G, K in ((1, 0), (32, 1), (255, 254), (32, 0)):
                got, recs = diff_map(a, b, mode=mode, gain=G, threshold=K, layout=layout)
                want = _ref(mode, a, b, G, K, layout)
                assert got.shape == want.shape and got.dtype == np.uint8
                for i, name in enumerate(names):
                    assert np.array_equal(got[i], want[i]), (name, mode, layout, G, K, H, W)
                    assert recs[i].astuple() == D.record(a[i], b[i], K), (name, mode, layout, G, K, H, W)
    one, rec = diff_map(a[1], b[1])  # one frame, every default: heat, G = 32, K = 1, the map alone
    assert np.array_equal(one, D.heat_map(a[1], b[1], 32, 1)) and rec.astuple() == D.record(a[1], b[1], 1)


@pytest.mark.parametrize("H,W", [(2, 16), (32, 64)])
@pytest.mark.parametrize("off_a,off_b,off_o", [(0, 0, 0), (1, 0, 0), (0, 16, 3), (16, 16, 16)])
def test_unaligned_buffers_take_the_block_path_at_a_vector_sized_frame(H, W, off_a, off_b, off_o):
    from animal_vision_amd.metrics import DIFF_RECORD_BYTES, diff_map_launch, diff_records_from_bytes
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    names, a, b = _pairs(H, W)
    n, fb = len(a), H * W * 3
    d_a, d_b, d_o, d_r = ctx.malloc(n * fb + 32), ctx.malloc(n * fb + 32), ctx.malloc(3 * n * fb + 32), ctx.malloc(n * DIFF_RECORD_BYTES)
    try:
        va, vb = d_a.view(off_a, n * fb), d_b.view(off_b, n * fb)
        ctx.upload(a, va)
        ctx.upload(b, vb)
        for mode, layout in (("heat", "map"), ("abs", "side")):
            wide = 3 if layout == "side" else 1
            vo = d_o.view(off_o, wide * n * fb)
            diff_map_launch(ctx, va, vb, n, H, W, vo, d_r, mode=mode, gain=32, threshold=1, layout=layout)
            got = ctx.download(vo, (n, H, W * wide, 3), np.uint8)
            recs = diff_records_from_bytes(ctx.download(d_r, (n * DIFF_RECORD_BYTES,), np.uint8), n)
            assert np.array_equal(got, _ref(mode, a, b, 32, 1, layout)), (mode, layout)
            assert [r.astuple() for r in recs] == [D.record(x, y, 1) for x, y in zip(a, b)]
    finally:
        for d in (d_a, d_b, d_o, d_r):
            d.free()


@pytest.mark.parametrize("H,W", [(32, 64), (37, 53), (75, 107)])
def test_planted_block(H, W):
    from animal_vision_amd.metrics import diff_map

    y0, x0 = H - 8, W // 2
    a, b = D.planted_pair(H, W, y0, x0)
    for layout in ("map", "side"):
        m, rec = diff_map(a, b, layout=layout)
        assert rec.astuple() == (7, x0, y0, 9)
        m = m[:, 2 * W:] if layout == "side" else m
        grey = (m[..., 0] == m[..., 1]) & (m[..., 1] == m[..., 2]) & (m[..., 0] < 64)
        hot = np.zeros((H, W), bool)
        hot[y0 : y0 + 3, x0 : x0 + 3] = True
        assert np.array_equal(~grey, hot)
        assert (m[hot] == D.pal(32 * 6)).all()
    if H >= 11 and W >= 11:
        _, rec = diff_map(a, b, mode="ssim", threshold=6)
        assert rec.astuple() == (7, x0, y0, 9)
        assert diff_map(a, b, mode="ssim", threshold=7)[1].astuple() == (7, x0, y0, 0)


# ------------------------------------------------------------------------------------------------ SSIM
@pytest.mark.parametrize("H,W", SSIM_SIZES)
def test_ssim_positions_within_the_float32_forms_own_error(H, W):
    from animal_vision_amd.metrics import ssim_map

    names, a, b = _pairs(H, W)
    pos, tol = _ssim_ref(H, W)
    got = ssim_map(a, b)
    assert got.dtype == np.float32 and got.shape == pos.shape
    dev = np.abs(got.astype(np.float64) - pos)
    print(f"ssim_map {H}x{W}: tol {tol:.3e}, largest deviation {dev.max():.3e} ({names[int(np.argmax(dev.reshape(len(names), -1).max(axis=1)))]})")
    assert dev.max() <= tol, (H, W, float(dev.max()), tol)


@pytest.mark.parametrize("H,W", SSIM_SIZES)
def test_mean_of_the_positions_is_the_record(H, W):
    from animal_vision_amd.metrics import frame_metrics, ssim_map

    names, a, b = _pairs(H, W)
    got = ssim_map(a, b)
    recs = frame_metrics(a, b)
    means = [got[i].astype(np.float64).reshape(-1, 3).sum(axis=0) / ((H - 10) * (W - 10)) for i in range(len(a))]
    worst = max(abs(means[i][c] - recs[i].ssim[c]) for i in range(len(a)) for c in range(3))
    print(f"ssim_map {H}x{W}: mean of the positions against the record: {worst:.3e}")
    for i, m in enumerate(recs):
        for c in range(3):
            assert abs(means[i][c] - m.ssim[c]) <= 1e-9, (names[i], H, W, c, means[i][c], m.ssim[c])


@pytest.mark.parametrize("H,W", SSIM_SIZES)
def test_ssim_mode_output(H, W):
    from animal_vision_amd.metrics import diff_map

    names, a, b = _pairs(H, W)
    pos, tol = _ssim_ref(H, W)
    yy, xx = np.clip(np.arange(H) - 5, 0, H - 11) + 5, np.clip(np.arange(W) - 5, 0, W - 11) + 5
    for G in (1.0, 4.0, 16.0):
        got, recs = diff_map(a, b, mode="ssim", gain=G, threshold=1)
        assert got.shape == (len(a), H, W, 3)
        v = got.astype(np.int64).sum(axis=-1)
        assert (v % 3 == 0).all() and np.array_equal(got, D.pal(v // 3)), G  # palette colours only: v is recovered exactly
        v = v // 3
        for i, name in enumerate(names):
            want = np.clip(D.replicate(D.ssim_v_unrounded(pos[i], G), H, W), 0.0, 255.0)
            assert (np.abs(v[i] - want) <= 0.5 + 255.0 * G * tol).all(), (name, G, H, W, float(np.abs(v[i] - want).max()))
            assert np.array_equal(got[i], got[i][yy][:, xx]), (name, G)  # a border pixel is its clamped position's pixel
            assert recs[i].astuple() == D.record(a[i], b[i], 1), (name, G)
        if (H, W) == (11, 11):
            assert all(len(np.unique(v[i])) == 1 for i in range(len(a)))  # one position: one value
    side, recs = diff_map(a, b, mode="ssim", layout="side")
    ref, _ = diff_map(a, b, mode="ssim")
    assert np.array_equal(side, D.side(a, b, ref))
    same, recs = diff_map(a, a, mode="ssim", gain=16.0, threshold=0)
    assert not same.any() and all(r.astuple() == (0, 0, 0, 0) for r in recs)


# ------------------------------------------------------------------------------------------------ batches
def test_batches_are_bit_equal_to_single_frames_and_repeatable():
    from animal_vision_amd.metrics import diff_map, ssim_map

    H, W = 75, 107  # 3 x 4 tiles, nothing aligned
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (16, H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    b[3:] = rng.integers(0, 256, (13, H, W, 3), dtype=np.uint8)  # every frame pair different
    for mode, layout in (("heat", "side"), ("ssim", "map")):
        single = [diff_map(a[i], b[i], mode=mode, layout=layout) for i in range(16)]
        for n in (1, 3, 16):
            got, recs = diff_map(a[16 - n:], b[16 - n:], mode=mode, layout=layout)
            again, recs2 = diff_map(a[16 - n:], b[16 - n:], mode=mode, layout=layout)
            assert len(got) == len(recs) == n
            for i in range(n):
                assert np.array_equal(got[i], single[16 - n + i][0]) and recs[i] == single[16 - n + i][1], (mode, n, i)
                assert np.array_equal(got[i], again[i]) and recs[i] == recs2[i], (mode, n, i)
        more, recs = diff_map(np.concatenate([a, a[:5]]), np.concatenate([b, b[:5]]), mode=mode, layout=layout)  # 21 frames: two chunks
        assert len(more) == len(recs) == 21
        assert all(np.array_equal(more[i], single[i % 16][0]) and recs[i] == single[i % 16][1] for i in range(21))
    single = [ssim_map(a[i], b[i])[0] for i in range(16)]
    for n in (1, 3, 16):
        got, again = ssim_map(a[16 - n:], b[16 - n:]), ssim_map(a[16 - n:], b[16 - n:])
        assert got.tobytes() == again.tobytes() and all(got[i].tobytes() == single[16 - n + i].tobytes() for i in range(n)), n
    more = ssim_map(np.concatenate([a, a[:5]]), np.concatenate([b, b[:5]]))
    assert all(more[i].tobytes() == single[i % 16].tobytes() for i in range(21))


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing():
    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import DIFF_RECORD_BYTES
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 16, 16
    fb = H * W * 3
    d_in = ctx.upload(np.zeros(3 * fb, np.uint8))  # a, b and room behind them, so that an overlapping output is still inside a buffer
    a, b = d_in.ptr, d_in.ptr + fb
    d_out = ctx.upload(np.full(3 * fb, 0xAB, np.uint8))
    d_rec = ctx.upload(np.full(DIFF_RECORD_BYTES, 0xAB, np.uint8))
    d_map = ctx.upload(np.full(6 * 6 * 3 * 4, 0xAB, np.uint8))
    o, r, m = d_out.ptr, d_rec.ptr, d_map.ptr
    fn = _lib.lib.avx_diff_map_u8
    HEAT, SSIM = 1, 2
    try:
        #         a     b     n  H  W  mode gain threshold layout out rec map
        for args in ((None, b, 1, H, W, HEAT, 32.0, 1, 0, o, r, None), (a, None, 1, H, W, HEAT, 32.0, 1, 0, o, r, None),
                     (a, b, 1, H, W, HEAT, 32.0, 1, 0, None, r, None), (a, b, 1, H, W, HEAT, 32.0, 1, 0, o, None, None),
                     (a, b, 0, H, W, HEAT, 32.0, 1, 0, o, r, None), (a, b, 17, H, W, HEAT, 32.0, 1, 0, o, r, None),
                     (a, b, 1, 0, W, HEAT, 32.0, 1, 0, o, r, None), (a, b, 1, H, -3, HEAT, 32.0, 1, 0, o, r, None),
                     (a, b, 1, 1 << 16, 1 << 16, HEAT, 32.0, 1, 0, o, r, None),
                     (a, b, 1, H, W, 3, 32.0, 1, 0, o, r, None), (a, b, 1, H, W, -1, 32.0, 1, 0, o, r, None),
                     (a, b, 1, H, W, HEAT, 32.0, 1, 2, o, r, None), (a, b, 1, H, W, HEAT, 32.0, 1, -1, o, r, None),
                     (a, b, 1, H, W, HEAT, 0.0, 1, 0, o, r, None), (a, b, 1, H, W, HEAT, 256.0, 1, 0, o, r, None),
                     (a, b, 1, H, W, HEAT, 2.5, 1, 0, o, r, None), (a, b, 1, H, W, 0, 0.5, 1, 0, o, r, None),
                     (a, b, 1, H, W, HEAT, float("nan"), 1, 0, o, r, None),
                     (a, b, 1, H, W, SSIM, 0.0, 1, 0, o, r, None), (a, b, 1, H, W, SSIM, 16.5, 1, 0, o, r, None),
                     (a, b, 1, H, W, SSIM, float("nan"), 1, 0, o, r, None),
                     (a, b, 1, H, W, HEAT, 32.0, -1, 0, o, r, None), (a, b, 1, H, W, HEAT, 32.0, 255, 0, o, r, None),
                     (a, b, 1, 10, W, SSIM, 4.0, 1, 0, o, r, None), (a, b, 1, H, 10, SSIM, 4.0, 1, 0, o, r, m),
                     (a, b, 1, H, W, HEAT, 32.0, 1, 0, o, r, m), (a, b, 1, H, W, 0, 32.0, 1, 0, o, r, m),
                     (a, b, 1, H, W, HEAT, 32.0, 1, 0, a, r, None), (a, b, 1, H, W, HEAT, 32.0, 1, 0, b + fb - 1, r, None),
                     (a, b, 1, H, W, HEAT, 32.0, 1, 1, a + fb, r, None), (a, a, 1, H, W, SSIM, 4.0, 1, 0, a + 1, r, None)):
            pa, pb, n, h, w, mode, gain, thr, layout, po, pr, pm = args
            rc = fn(ctx._h, pa, pb, n, h, w, mode, gain, thr, layout, po, pr, pm, ctx.stream)
            assert rc == _lib.AVX_ERR_INVALID, args
            assert _lib.lib.avx_last_error(ctx._h).decode().startswith("avx_diff_map_u8:"), args
        ctx.sync()
        assert (ctx.download(d_out, (3 * fb,), np.uint8) == 0xAB).all() and (ctx.download(d_rec, (DIFF_RECORD_BYTES,), np.uint8) == 0xAB).all()
        assert (ctx.download(d_map, (6 * 6 * 3 * 4,), np.uint8) == 0xAB).all() and not ctx.download(d_in, (3 * fb,), np.uint8).any()
        ctx.upload(np.ones(fb, np.uint8), d_in.view(fb, fb))  # b = a + 1: the good call still works
        assert fn(ctx._h, a, b, 1, H, W, SSIM, 4.0, 0, 1, o, r, m, ctx.stream) == 0
        rec = np.frombuffer(ctx.download(d_rec, (DIFF_RECORD_BYTES,), np.uint8).tobytes(), np.uint32)
        assert rec.tolist() == [1, 0, 0, H * W]
        out = ctx.download(d_out, (H, 3 * W, 3), np.uint8)
        assert not out[:, :W].any() and (out[:, W : 2 * W] == 1).all()
        assert np.isfinite(ctx.download(d_map, (6, 6, 3), np.float32)).all()
    finally:
        for d in (d_in, d_out, d_rec, d_map):
            d.free()


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from animal_vision_amd.renderers import VideoRenderer

    d = tmp_path_factory.mktemp("diff_clips")
    rng = np.random.default_rng(11)
    base = np.kron(rng.integers(0, 256, (12, 12, 16, 3), dtype=np.uint8), np.ones((1, 4, 4, 1), np.uint8))  # 48 x 64 blocks
    a = np.clip(base.astype(np.int16) + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-3, 4, a.shape) * (rng.random(a.shape[:3] + (1,)) < 0.1), 0, 255).astype(np.uint8)
    np.save(d / "a.npy", a)
    np.save(d / "b.npy", b)
    np.save(d / "b9.npy", b[:9])
    for name, fmt, frames in (("a.y4m", None, a), ("b.y4m", None, b), ("a.nv12.yuv", "nv12", a), ("b.nv12.yuv", "nv12", b)):
        vr = VideoRenderer(read_path=None, write_path=str(d / name), write_pix_fmt=fmt)
        vr.open()
        for f in frames:
            vr.render(f)
        vr.close()
    return d, a, b


def _diff(capsys, argv):
    from animal_vision_amd import diff

    status = diff.main([str(v) for v in argv])
    cap = capsys.readouterr()
    return status, cap.out, cap.err


def _y4m_frames(path):
    """(header fields, [payload bytes]) of a .y4m file, read by hand."""
    data = open(path, "rb").read()
    end = data.index(b"\n")
    fields = data[:end].split(b" ")
    W, H = (int(next(f for f in fields if f[:1] == k)[1:]) for k in (b"W", b"H"))
    fsz = H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
    frames, p = [], end + 1
    while p < len(data):
        assert data[p : p + 6] == b"FRAME\n"
        frames.append(np.frombuffer(data[p + 6 : p + 6 + fsz], np.uint8))
        p += 6 + fsz
    return (W, H), frames


def test_command_npy_sink_and_csv(clips, capsys, tmp_path):
    from animal_vision_amd.diff import CSV_HEADER, format_row
    from animal_vision_amd.metrics import diff_map

    d, a, b = clips
    for extra, kw in (([], {}), (["--mode", "abs", "--gain", "64", "--layout", "side", "--batch", "5", "--depth", "3"], dict(mode="abs", gain=64, layout="side")),
                      (["--mode", "ssim", "--threshold", "2", "--depth", "1"], dict(mode="ssim", threshold=2))):
        out, csv = tmp_path / "o.npy", tmp_path / "w.csv"
        status, stdout, err = _diff(capsys, [d / "a.npy", d / "b.npy", out, "--csv", csv] + extra)
        want, recs = diff_map(a, b, **kw)
        assert status == 0 and stdout == "" and "diff: 12 frames" in err
        assert np.array_equal(np.load(out), want), extra
        assert csv.read_text() == CSV_HEADER + "\n" + "".join(format_row(i, r) + "\n" for i, r in enumerate(recs)), extra
        worst = max(r.max_d for r in recs)
        first = next(i for i, r in enumerate(recs) if r.max_d == worst)
        assert f"largest difference {worst} (frame {first}, pixel x {recs[first].max_x} y {recs[first].max_y})" in err
        assert f"{sum(r.beyond for r in recs)} pixels beyond {kw.get('threshold', 1)}" in err


def test_command_encoded_sinks(clips, capsys, tmp_path):
    import _rawyuv_ref
    import _yuv_ref
    from animal_vision_amd.metrics import diff_map

    d, a, b = clips
    want, _ = diff_map(a, b)
    status, _, _ = _diff(capsys, [d / "a.npy", d / "b.npy", tmp_path / "o.y4m"])
    (W, H), frames = _y4m_frames(tmp_path / "o.y4m")
    assert status == 0 and (W, H) == (64, 48) and len(frames) == 12
    assert np.array_equal(np.stack(frames), _yuv_ref.encode(want))
    side, _ = diff_map(a, b, layout="side")
    status, _, _ = _diff(capsys, [d / "a.npy", d / "b.npy", tmp_path / "s.y4m", "--layout", "side", "--batch", "16"])
    (W, H), frames = _y4m_frames(tmp_path / "s.y4m")
    assert status == 0 and (W, H) == (192, 48) and np.array_equal(np.stack(frames), _yuv_ref.encode(side))
    status, _, _ = _diff(capsys, [d / "a.npy", d / "b.npy", tmp_path / "o.yuv", "--out-pix-fmt", "nv12"])
    raw = np.fromfile(tmp_path / "o.yuv", np.uint8).reshape(12, -1)
    assert status == 0 and np.array_equal(raw, _rawyuv_ref.encode(want, "nv12"))


def test_command_payload_inputs_equal_the_get_image_route(clips, capsys, tmp_path):
    from animal_vision_amd.metrics import diff_map
    from animal_vision_amd.renderers import VideoRenderer

    d, a, b = clips

    def decoded(path, opts):
        vr = VideoRenderer(read_path=str(path), pix_fmt="nv12" if opts else None, size=(64, 48) if opts else None)
        vr.open()
        frames = np.stack([vr.get_image() for _ in range(12)])
        assert vr.get_image() is None
        vr.close()
        return frames

    for na, nb, opts in (("a.y4m", "b.y4m", []), ("a.nv12.yuv", "b.nv12.yuv", ["--pix-fmt", "nv12", "--size", "64x48"])):
        da, db = decoded(d / na, opts), decoded(d / nb, opts)
        assert not np.array_equal(da, a) and not np.array_equal(da, db)  # 4:2:0 is lossy, and there is something to show
        want, recs = diff_map(da, db, threshold=0)
        out = tmp_path / (na + ".npy")
        status, _, _ = _diff(capsys, [d / na, d / nb, out, "--threshold", "0", "--batch", "5"] + opts)
        assert status == 0 and np.array_equal(np.load(out), want), na
    # a payload input against a get_image() input
    da = decoded(d / "a.y4m", [])
    status, _, _ = _diff(capsys, [d / "a.y4m", d / "b.npy", tmp_path / "mixed.npy", "--mode", "abs"])
    assert status == 0 and np.array_equal(np.load(tmp_path / "mixed.npy"), diff_map(da, b, mode="abs")[0])


def test_command_lengths_and_sizes(clips, capsys, tmp_path):
    d, a, b = clips
    status, _, err = _diff(capsys, [d / "a.npy", d / "b9.npy", tmp_path / "o.npy"])
    assert status == 2 and "A has more frames" in err and len(np.load(tmp_path / "o.npy")) == 9
    status, _, err = _diff(capsys, [d / "b9.npy", d / "a.npy", tmp_path / "p.npy", "--shortest", "--batch", "3"])  # the shorter one ends on a batch boundary
    assert status == 0 and "more frames" not in err and len(np.load(tmp_path / "p.npy")) == 9
    np.save(tmp_path / "small.npy", a[:2, :40])
    with pytest.raises(SystemExit, match="frame sizes differ"):
        _diff(capsys, [d / "a.npy", tmp_path / "small.npy", tmp_path / "q.npy"])
    np.save(tmp_path / "tiny.npy", a[:2, :10, :30])
    with pytest.raises(SystemExit, match="--mode ssim needs frames of at least 11x11; these are 30x10"):
        _diff(capsys, [tmp_path / "tiny.npy", tmp_path / "tiny.npy", tmp_path / "r.npy", "--mode", "ssim"])


def test_command_output_does_not_depend_on_batch_and_depth(capsys, tmp_path):
    """The shared device loop (pairs.stream_pairs): the maps and the CSV are the same bytes however the nine frames are cut into
    batches and spread over buffer sets -- one set, three sets, a batch per frame, the whole clip in one batch."""
    got = []
    for batch, depth in ((8, 2), (1, 1), (3, 3), (9, 1)):
        out, csv = tmp_path / f"o_{batch}_{depth}.npy", tmp_path / f"w_{batch}_{depth}.csv"
        status, stdout, err = _diff(capsys, ["synthetic:64x48:9:noise", "synthetic:64x48:9:structured", out, "--csv", csv, "--batch", batch, "--depth", depth])
        assert status == 0 and stdout == "" and "diff: 9 frames" in err
        got.append((out.read_bytes(), csv.read_bytes()))
    assert np.load(tmp_path / "o_8_2.npy").shape == (9, 48, 64, 3) and np.load(tmp_path / "o_8_2.npy").any()
    assert len(got[0][1].splitlines()) == 10
    for other in got[1:]:
        assert other == got[0]
