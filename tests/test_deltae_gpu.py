"""GPU: the colour difference kernel (csrc/delta_e.hip) against the float64 definition of tests/_deltae_ref.py, and the
deltae command end to end.  Small frames only: 5 x 7 is less than one vector, 29 x 37 is odd and on the byte path, 48 x 64 is on the
16-byte path, 72 x 64 and 67 x 71 are the two paths with more than one workgroup (a workgroup owns 4096 pixels).

Accuracy.  The device's float32 dE of every pixel is held to BOUND against the float64 yardstick.  Pixels whose yardstick hues satisfy
| |h'1 - h'2| - 180 | < 1e-3 degrees are left out (the mean-hue rule is discontinuous there and either side is a correct evaluation);
more than 0.1 % of a frame left out fails (none is, on these frames).  Measured on an MI355X on the frames of this file: the largest
|device - yardstick| is 7.85e-5 (frame pair "near" at 67 x 71; 5.92e-5 at 48 x 64, 4.62e-5 at 29 x 37, 2.09e-5 at 5 x 7; 1.7e-5 on the
greys against saturated colours, 1.5e-5 on the cube's corners); BOUND is the next power of ten above twice that, 1e-3.  For
orientation, a NumPy float32 restatement of the same arithmetic on a CPU is within 2.3e-4 on 10^6 random pairs.

Everything else has no tolerance: the record and the map are checked against the device's own float32 values -- the histogram of
floor(2 v), the first raster maximum, the count of v > T, the map as the yardstick's float32 quantiser of v -- and the float64 sum to a
relative 1e-12 (another order of the same float32 numbers in float64)."""
import numpy as np
import pytest

import _deltae_ref as E
from animal_vision_amd import deltae as _deltae_module  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu

BOUND = 1e-3
SHAPES = [(5, 7), (29, 37), (48, 64)]
TWO_BLOCKS = [(72, 64), (67, 71)]  # 4608 pixels on the 16-byte path, 4757 on the byte path
_cache = {}


def _frames(H, W):
    """The frame pairs of a size as two stacks, their names, the float64 yardstick and the left-out pixels; computed once, read-only."""
    if (H, W) not in _cache:
        named = E.frames(H, W, seed=H * 1000 + W)
        a, b = np.stack([p[1] for p in named]), np.stack([p[2] for p in named])
        want, out = E.delta_e(a, b), E.hue_ambiguous(a, b)
        for x in (a, b, want, out):
            x.setflags(write=False)
        _cache[(H, W)] = ([p[0] for p in named], a, b, want, out)
    return _cache[(H, W)]


def _check_record(rec, v, T, what):
    want = E.record(v, T)
    assert np.array_equal(rec.hist, want["hist"]), what
    assert (np.float32(rec.max_de).tobytes(), rec.max_x, rec.max_y) == (np.float32(want["max_de"]).tobytes(), want["max_x"], want["max_y"]), what
    assert rec.beyond == want["beyond"], what
    assert abs(rec.sum - want["sum"]) <= 1e-12 * max(want["sum"], 1e-300), (what, rec.sum, want["sum"])
    assert rec.pixels == v.size and rec.mean == rec.sum / v.size
    for q in (0.5, 0.95, 1.0):
        assert rec.percentile(q) == E.percentile(want["hist"], want["max_de"], q), (what, q)


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("H,W", SHAPES + TWO_BLOCKS)
def test_values_against_the_float64_definition(H, W):
    from animal_vision_amd.metrics import delta_e_values

    names, a, b, want, out = _frames(H, W)
    got = delta_e_values(a, b)
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and (got >= 0).all()
    dev = np.where(out, 0.0, np.abs(got.astype(np.float64) - want))
    for i, name in enumerate(names):
        print(f"delta_e {H}x{W} {name}: largest |device - yardstick| {dev[i].max():.3e}, left out {int(out[i].sum())} of {H * W}, largest dE {want[i].max():.4f}")
    for i, name in enumerate(names):
        assert out[i].mean() <= 1e-3, (name, H, W, int(out[i].sum()))
        assert dev[i].max() <= BOUND, (name, H, W, float(dev[i].max()))
    one = delta_e_values(a[1], b[1])  # one frame: H x W
    assert one.shape == (H, W) and one.tobytes() == got[1].tobytes()


def test_published_code_pairs_and_greys():
    from animal_vision_amd.metrics import delta_e_values

    a = np.array([[[0, 0, 0], [0, 0, 255], [0, 255, 0], [128, 128, 128], [128, 128, 128]]], np.uint8)
    b = np.array([[[255, 255, 255], [255, 255, 0], [255, 0, 255], [128, 129, 128], [0, 0, 255]]], np.uint8)
    got = delta_e_values(a, b)[0].astype(np.float64)
    assert np.abs(got[:3] - [100.0, 103.4270, 111.4143]).max() <= 1e-4 + BOUND
    assert np.abs(got - E.delta_e(a, b)[0]).max() <= BOUND
    assert 0.67 <= got[3] <= 1.23
    # every grey against every other grey: no chroma anywhere, dE is a function of L alone and symmetric bit for bit
    g = np.arange(256, dtype=np.uint8)
    ga, gb = np.repeat(np.repeat(g[:, None], 256, axis=1)[..., None], 3, axis=2), np.repeat(np.repeat(g[None, :], 256, axis=0)[..., None], 3, axis=2)
    v = delta_e_values(ga, gb)
    assert np.abs(v.astype(np.float64) - E.delta_e(ga, gb)).max() <= BOUND
    assert v.tobytes() == v.T.copy().tobytes() and (np.diag(v) == 0).all()


# ------------------------------------------------------------------------------------------------ the record and the map: no tolerance
@pytest.mark.parametrize("H,W", SHAPES + TWO_BLOCKS)
def test_record_and_map_follow_the_devices_own_values(H, W):
    from animal_vision_amd.metrics import delta_e, delta_e_map, delta_e_values

    names, a, b, _, _ = _frames(H, W)
    v = delta_e_values(a, b)
    for mode, layout, G, T in (("heat", "map", None, 1.0), ("heat", "side", 10.0, 1.0), ("plain", "map", 10.0, 1.0), ("plain", "side", 2.5, 0.0),
                               ("heat", "map", 255.0, 0.0), ("heat", "side", 0.37, 2.3), ("plain", "map", 1.0, 50.0)):
        got, recs = delta_e_map(a, b, mode=mode, gain=G, threshold=T, layout=layout)
        assert got.dtype == np.uint8 and got.shape == (len(a), H, W * (3 if layout == "side" else 1), 3)
        only = delta_e(a, b, threshold=T)
        for i, name in enumerate(names):
            what = (name, mode, layout, G, T, H, W)
            m = E.de_map(v[i], a[i], 10.0 if G is None else G, T, mode)
            assert np.array_equal(got[i], E.side(a[i], b[i], m) if layout == "side" else m), what
            _check_record(recs[i], v[i], T, what)
            assert only[i] == recs[i], what  # records only (no map) is the same record
    one, rec = delta_e_map(a[0], b[0])  # one frame, every default: heat, G = 10, T = 1, the map alone
    assert np.array_equal(one, E.de_map(v[0], a[0], 10.0, 1.0, "heat")) and rec == delta_e(a[0], b[0])


@pytest.mark.parametrize("H,W", [(29, 37), (48, 64)] + TWO_BLOCKS)
def test_the_first_of_two_equal_maxima_is_reported(H, W):
    from animal_vision_amd.metrics import delta_e_map, delta_e_values

    a = np.full((H, W, 3), 100, np.uint8)
    a[..., 1] = (np.arange(H * W).reshape(H, W) % 7 + 97).astype(np.uint8)  # not flat: the small differences below are not all one value
    b = a.copy()
    b[..., 2] += 1
    first, second = (H // 3, W - 2), (H - 1, 1)  # in raster order; in different workgroups where the frame has two
    for y, x in (first, second):
        a[y, x], b[y, x] = (100, 100, 100), (100, 100, 255)
    v = delta_e_values(a, b)
    assert v[first] == v[second] == v.max() and (v == v.max()).sum() == 2 and v.max() > 30
    for layout in ("map", "side"):
        m, rec = delta_e_map(a, b, layout=layout)
        assert (rec.max_x, rec.max_y) == (first[1], first[0]) and np.float32(rec.max_de) == v.max()
        _check_record(rec, v, 1.0, (H, W, layout))
    _, rec = delta_e_map(b[::-1, ::-1].copy(), a[::-1, ::-1].copy())  # mirrored: the other pixel comes first
    assert (rec.max_x, rec.max_y) == (W - 1 - second[1], H - 1 - second[0])


# ------------------------------------------------------------------------------------------------ exact and invariant cases
@pytest.mark.parametrize("H,W", SHAPES + TWO_BLOCKS)
def test_identical_frames_are_exactly_zero(H, W):
    from animal_vision_amd.metrics import delta_e_map, delta_e_values

    _, a, _, _, _ = _frames(H, W)
    v = delta_e_values(a, a)
    assert not v.any() and v.dtype == np.float32
    plain, recs = delta_e_map(a, a, mode="plain", gain=255.0, threshold=0.0)
    assert not plain.any()
    heat, recs_h = delta_e_map(a, a, mode="heat", gain=255.0, threshold=0.0, layout="side")
    x = a.astype(np.int64)
    g = (((77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8) >> 2).astype(np.uint8)
    assert np.array_equal(heat[:, :, 2 * W:], np.stack([g, g, g], axis=-1)) and np.array_equal(heat[:, :, :W], a) and np.array_equal(heat[:, :, W : 2 * W], a)
    for r in recs + recs_h:
        assert r.hist[0] == H * W and r.hist.sum() == H * W and (r.sum, r.max_de, r.max_x, r.max_y, r.beyond) == (0.0, 0.0, 0, 0, 0)
        assert r.mean == 0.0 and r.percentile(0.95) == 0.5


@pytest.mark.parametrize("H,W", [(29, 37)] + TWO_BLOCKS)
def test_batches_are_bit_equal_to_single_frames_and_repeatable(H, W):
    from animal_vision_amd.metrics import delta_e_map, delta_e_values

    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (16, H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    b[3:] = rng.integers(0, 256, (13, H, W, 3), dtype=np.uint8)  # every frame pair different
    single = [delta_e_map(a[i], b[i], layout="side") + (delta_e_values(a[i], b[i]),) for i in range(16)]
    for n in (1, 3, 16):
        for lo in sorted({0, 16 - n}):  # the frames in other slots of the batch
            got, recs = delta_e_map(a[lo : lo + n], b[lo : lo + n], layout="side")
            again, recs2 = delta_e_map(a[lo : lo + n], b[lo : lo + n], layout="side")
            vals, vals2 = delta_e_values(a[lo : lo + n], b[lo : lo + n]), delta_e_values(a[lo : lo + n], b[lo : lo + n])
            assert len(got) == len(recs) == len(vals) == n and vals.tobytes() == vals2.tobytes()
            for i in range(n):
                m, r, v = single[lo + i]
                assert np.array_equal(got[i], m) and recs[i] == r and vals[i].tobytes() == v.tobytes(), (n, lo, i)
                assert np.array_equal(got[i], again[i]) and recs[i] == recs2[i], (n, lo, i)
    # a frame in any slot of a batch of 16
    for slot in (0, 7, 15):
        aa, bb = np.roll(a, slot, axis=0), np.roll(b, slot, axis=0)
        got, recs = delta_e_map(aa, bb, layout="side")
        assert np.array_equal(got[slot], single[0][0]) and recs[slot] == single[0][1]
        assert delta_e_values(aa, bb)[slot].tobytes() == single[0][2].tobytes()
    more, recs = delta_e_map(np.concatenate([a, a[:5]]), np.concatenate([b, b[:5]]), layout="side")  # 21 frames: two chunks
    assert len(more) == len(recs) == 21
    assert all(np.array_equal(more[i], single[i % 16][0]) and recs[i] == single[i % 16][1] for i in range(21))


@pytest.mark.parametrize("off", [1, 4, 8])
def test_unaligned_buffers_take_the_byte_path_at_a_vector_sized_frame(off):
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, delta_e_launch, delta_e_map, delta_e_records_from_bytes, delta_e_values
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 48, 64
    names, a, b, want, out = _frames(H, W)
    n, fb = len(a), H * W * 3
    v0 = delta_e_values(a, b)  # everything aligned: the 16-byte path
    d_a, d_b, d_o, d_r, d_v = ctx.malloc(n * fb + 32), ctx.malloc(n * fb + 32), ctx.malloc(3 * n * fb + 32), ctx.malloc(n * DELTA_E_RECORD_BYTES), ctx.malloc(n * H * W * 4)
    try:
        for off_a, off_b, off_o in ((off, off, off), (off, 0, 0), (0, off, 0), (0, 0, off)):
            va, vb = d_a.view(off_a, n * fb), d_b.view(off_b, n * fb)
            ctx.upload(a, va)
            ctx.upload(b, vb)
            for mode, layout in (("heat", "map"), ("plain", "side")):
                wide = 3 if layout == "side" else 1
                vo = d_o.view(off_o, wide * n * fb)
                delta_e_launch(ctx, va, vb, n, H, W, vo, d_r, mode=mode, layout=layout, d_float=d_v)
                got = ctx.download(vo, (n, H, W * wide, 3), np.uint8)
                recs = delta_e_records_from_bytes(ctx.download(d_r, (n * DELTA_E_RECORD_BYTES,), np.uint8), n)
                v = ctx.download(d_v, (n, H, W), np.float32)
                assert np.where(out, 0.0, np.abs(v.astype(np.float64) - want)).max() <= BOUND
                assert v.tobytes() == v0.tobytes(), (off_a, off_b, off_o)  # one arithmetic, whatever the path
                ref_map, ref_recs = delta_e_map(a, b, mode=mode, layout=layout)
                assert np.array_equal(got, ref_map) and recs == ref_recs, (mode, layout, off_a, off_b, off_o)
                for i, name in enumerate(names):
                    m = E.de_map(v[i], a[i], 10.0, 1.0, mode)
                    assert np.array_equal(got[i], E.side(a[i], b[i], m) if layout == "side" else m), (name, mode, layout)
                    _check_record(recs[i], v[i], 1.0, (name, mode, layout, off))
    finally:
        for d in (d_a, d_b, d_o, d_r, d_v):
            d.free()


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing():
    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, delta_e_records_from_bytes
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 16, 16
    fb = H * W * 3
    d_in = ctx.upload(np.zeros(3 * fb, np.uint8))  # a, b and room behind them, so that an overlapping output is still inside a buffer
    a, b = d_in.ptr, d_in.ptr + fb
    d_out = ctx.upload(np.full(3 * fb, 0xAB, np.uint8))
    d_rec = ctx.upload(np.full(DELTA_E_RECORD_BYTES + 8, 0xAB, np.uint8))
    d_val = ctx.upload(np.full(H * W * 4 + 4, 0xAB, np.uint8))
    o, r, v = d_out.ptr, d_rec.ptr, d_val.ptr
    fn = _lib.lib.avx_delta_e_u8
    HEAT, PLAIN = 0, 1
    nan, inf = float("nan"), float("inf")
    try:
        #         a     b     n  H  W  mode gain threshold layout map rec values
        for args in ((None, b, 1, H, W, HEAT, 10.0, 1.0, 0, o, r, v), (a, None, 1, H, W, HEAT, 10.0, 1.0, 0, o, r, v),
                     (a, b, 1, H, W, HEAT, 10.0, 1.0, 0, o, None, v),
                     (a, b, 0, H, W, HEAT, 10.0, 1.0, 0, o, r, v), (a, b, 17, H, W, HEAT, 10.0, 1.0, 0, o, r, v), (a, b, -1, H, W, HEAT, 10.0, 1.0, 0, o, r, v),
                     (a, b, 1, 0, W, HEAT, 10.0, 1.0, 0, o, r, v), (a, b, 1, H, -3, HEAT, 10.0, 1.0, 0, o, r, v),
                     (a, b, 1, 1 << 16, 1 << 16, HEAT, 10.0, 1.0, 0, o, r, v),
                     (a, b, 1, H, W, 2, 10.0, 1.0, 0, o, r, v), (a, b, 1, H, W, -1, 10.0, 1.0, 0, o, r, v),
                     (a, b, 1, H, W, HEAT, 10.0, 1.0, 2, o, r, v), (a, b, 1, H, W, PLAIN, 10.0, 1.0, -1, o, r, v),
                     (a, b, 1, H, W, HEAT, 0.0, 1.0, 0, o, r, v), (a, b, 1, H, W, HEAT, -1.0, 1.0, 0, o, r, v), (a, b, 1, H, W, PLAIN, 255.5, 1.0, 0, o, r, v),
                     (a, b, 1, H, W, HEAT, nan, 1.0, 0, o, r, v), (a, b, 1, H, W, HEAT, inf, 1.0, 0, o, r, v),
                     (a, b, 1, H, W, HEAT, 10.0, -0.5, 0, o, r, v), (a, b, 1, H, W, HEAT, 10.0, nan, 0, o, r, v), (a, b, 1, H, W, PLAIN, 10.0, inf, 0, o, r, v),
                     (a, b, 1, H, W, HEAT, 10.0, 1.0, 0, o, r + 4, v), (a, b, 1, H, W, HEAT, 10.0, 1.0, 0, o, r, v + 2),
                     (a, b, 1, H, W, HEAT, 10.0, 1.0, 0, a, r, v), (a, b, 1, H, W, HEAT, 10.0, 1.0, 0, b + fb - 1, r, v),
                     (a, b, 1, H, W, HEAT, 10.0, 1.0, 1, a + fb, r, v)):
            pa, pb, n, h, w, mode, gain, thr, layout, po, pr, pv = args
            rc = fn(ctx._h, pa, pb, n, h, w, mode, gain, thr, layout, po, pr, pv, ctx.stream)
            assert rc == _lib.AVX_ERR_INVALID, args
            assert _lib.lib.avx_last_error(ctx._h).decode().startswith("avx_delta_e_u8:"), args
        assert fn(None, a, b, 1, H, W, HEAT, 10.0, 1.0, 0, o, r, v, ctx.stream) == _lib.AVX_ERR_INVALID  # a NULL context
        ctx.sync()
        assert (ctx.download(d_out, (3 * fb,), np.uint8) == 0xAB).all() and (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8) == 0xAB).all()
        assert (ctx.download(d_val, (H * W * 4 + 4,), np.uint8) == 0xAB).all() and not ctx.download(d_in, (3 * fb,), np.uint8).any()
        ctx.upload(np.full(fb, 255, np.uint8), d_in.view(fb, fb))  # b = white against a = black: the good call still works
        assert fn(ctx._h, a, b, 1, H, W, PLAIN, 2.0, 1.0, 1, o, r, v, ctx.stream) == 0
        rec = delta_e_records_from_bytes(ctx.download(d_rec, (DELTA_E_RECORD_BYTES,), np.uint8), 1)[0]
        assert rec.hist[199] + rec.hist[200] == H * W and abs(rec.max_de - 100.0) <= BOUND and (rec.max_x, rec.max_y, rec.beyond) == (0, 0, H * W)
        out = ctx.download(d_out, (H, 3 * W, 3), np.uint8)
        assert not out[:, :W].any() and (out[:, W : 2 * W] == 255).all() and (out[:, 2 * W:] == E.pal(200)).all()
        assert (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8)[DELTA_E_RECORD_BYTES:] == 0xAB).all()  # nothing behind the record
        # records only: NULL map and NULL values are a good call
        assert fn(ctx._h, a, b, 1, H, W, HEAT, 10.0, 1.0, 0, None, r, None, ctx.stream) == 0
        assert delta_e_records_from_bytes(ctx.download(d_rec, (DELTA_E_RECORD_BYTES,), np.uint8), 1)[0] == rec
    finally:
        for d in (d_in, d_out, d_rec, d_val):
            d.free()


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from animal_vision_amd.renderers import VideoRenderer

    d = tmp_path_factory.mktemp("deltae_clips")
    rng = np.random.default_rng(11)
    base = np.kron(rng.integers(0, 256, (12, 12, 16, 3), dtype=np.uint8), np.ones((1, 4, 4, 1), np.uint8))  # 48 x 64 blocks
    a = np.clip(base.astype(np.int16) + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-3, 4, a.shape) * (rng.random(a.shape[:3] + (1,)) < 0.1), 0, 255).astype(np.uint8)
    b[5, 10:20, 30:40] = 255 - b[5, 10:20, 30:40]  # frame 5 carries a patch that is far off
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


def _deltae(capsys, argv):
    from animal_vision_amd import deltae

    status = deltae.main([str(v) for v in argv])
    cap = capsys.readouterr()
    return status, cap.out, cap.err


def _rows(recs):
    from animal_vision_amd.deltae import CSV_HEADER, format_row

    return CSV_HEADER + "\n" + "".join(format_row(i, r) + "\n" for i, r in enumerate(recs))


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


def test_command_npy_sink_csv_and_stdout(clips, capsys, tmp_path):
    from animal_vision_amd.pairs import num as _num
    from animal_vision_amd.metrics import delta_e, delta_e_map

    d, a, b = clips
    for extra, kw in (([], {}), (["--mode", "plain", "--gain", "4", "--layout", "side", "--batch", "5", "--depth", "3"], dict(mode="plain", gain=4, layout="side")),
                      (["--threshold", "2.5", "--depth", "1"], dict(threshold=2.5))):
        out, csv = tmp_path / "o.npy", tmp_path / "w.csv"
        status, stdout, err = _deltae(capsys, [d / "a.npy", d / "b.npy", out, "--csv", csv] + extra)
        want, recs = delta_e_map(a, b, **kw)
        assert status == 0 and stdout == "" and "deltae: 12 frames" in err
        assert np.array_equal(np.load(out), want), extra
        assert csv.read_text() == _rows(recs), extra
        worst = max(r.max_de for r in recs)
        first = next(i for i, r in enumerate(recs) if r.max_de == worst)
        assert first == 5 and f"largest dE {_num(worst)} (frame 5, pixel x {recs[5].max_x} y {recs[5].max_y})" in err
        assert f"mean dE {_num(sum(r.mean for r in recs) / 12)}" in err
        assert f"{sum(r.beyond for r in recs)} pixels beyond {kw.get('threshold', 1):g}" in err
    # without OUT: the same lines on stdout (no map is computed), or in --csv
    recs = delta_e(a, b)
    assert recs == delta_e_map(a, b)[1]
    status, stdout, err = _deltae(capsys, [d / "a.npy", d / "b.npy"])
    assert status == 0 and stdout == _rows(recs) and "deltae: 12 frames" in err
    status, stdout, err = _deltae(capsys, [d / "a.npy", d / "b.npy", "--csv", tmp_path / "only.csv", "--batch", "5", "--threshold", "2.5"])
    assert status == 0 and stdout == "" and (tmp_path / "only.csv").read_text() == _rows(delta_e(a, b, threshold=2.5))


def test_command_encoded_sinks(clips, capsys, tmp_path):
    import _rawyuv_ref
    import _yuv_ref
    from animal_vision_amd.metrics import delta_e_map

    d, a, b = clips
    want, _ = delta_e_map(a, b)
    status, _, _ = _deltae(capsys, [d / "a.npy", d / "b.npy", tmp_path / "o.y4m"])
    (W, H), frames = _y4m_frames(tmp_path / "o.y4m")
    assert status == 0 and (W, H) == (64, 48) and len(frames) == 12
    assert np.array_equal(np.stack(frames), _yuv_ref.encode(want))
    side, recs = delta_e_map(a, b, layout="side")
    status, _, _ = _deltae(capsys, [d / "a.npy", d / "b.npy", tmp_path / "s.y4m", "--layout", "side", "--batch", "16", "--csv", tmp_path / "s.csv"])
    (W, H), frames = _y4m_frames(tmp_path / "s.y4m")
    assert status == 0 and (W, H) == (192, 48) and np.array_equal(np.stack(frames), _yuv_ref.encode(side))
    assert (tmp_path / "s.csv").read_text() == _rows(recs)
    status, _, _ = _deltae(capsys, [d / "a.npy", d / "b.npy", tmp_path / "o.yuv", "--out-pix-fmt", "nv12"])
    raw = np.fromfile(tmp_path / "o.yuv", np.uint8).reshape(12, -1)
    assert status == 0 and np.array_equal(raw, _rawyuv_ref.encode(want, "nv12"))


def test_command_payload_inputs_equal_the_get_image_route(clips, capsys, tmp_path):
    from animal_vision_amd.metrics import delta_e, delta_e_map
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
        want, recs = delta_e_map(da, db, threshold=0.5)
        out = tmp_path / (na + ".npy")
        status, _, _ = _deltae(capsys, [d / na, d / nb, out, "--threshold", "0.5", "--batch", "5"] + opts)
        assert status == 0 and np.array_equal(np.load(out), want), na
        status, stdout, _ = _deltae(capsys, [d / na, d / nb, "--threshold", "0.5"] + opts)
        assert status == 0 and stdout == _rows(recs), na
    # a payload input against a get_image() input
    da = decoded(d / "a.y4m", [])
    status, stdout, _ = _deltae(capsys, [d / "a.y4m", d / "b.npy"])
    assert status == 0 and stdout == _rows(delta_e(da, b))


def test_command_lengths_sizes_and_limits(clips, capsys, tmp_path):
    from animal_vision_amd.metrics import delta_e

    d, a, b = clips
    status, _, err = _deltae(capsys, [d / "a.npy", d / "b9.npy", tmp_path / "o.npy"])
    assert status == 2 and "A has more frames" in err and len(np.load(tmp_path / "o.npy")) == 9
    status, stdout, err = _deltae(capsys, [d / "b9.npy", d / "a.npy", "--shortest", "--batch", "3"])  # the shorter one ends on a batch boundary
    assert status == 0 and "more frames" not in err and len(stdout.splitlines()) == 10
    np.save(tmp_path / "small.npy", a[:2, :40])
    with pytest.raises(SystemExit, match="deltae: frame sizes differ: A is 64x48, B is 64x40"):
        _deltae(capsys, [d / "a.npy", tmp_path / "small.npy", tmp_path / "q.npy"])
    assert not (tmp_path / "q.npy").exists()  # nothing is written before the sizes are known to agree
    recs = delta_e(a, b)
    quiet = max(max(r.max_de for i, r in enumerate(recs) if i != 5), 1.0)
    assert recs[5].max_de > quiet + 1 and recs[5].mean > max(r.mean for i, r in enumerate(recs) if i != 5)
    mean_limit = (recs[5].mean + max(r.mean for i, r in enumerate(recs) if i != 5)) / 2
    for argv, text in ((["--max-de", f"{quiet + 0.5:.3f}"], "deltae: frame 5: largest dE"), (["--max-mean", f"{mean_limit:.6f}"], "deltae: frame 5: mean dE"),
                       (["--max-p95", "0.25"], "deltae: frame 0: 95th percentile dE")):
        status, stdout, err = _deltae(capsys, [d / "a.npy", d / "b.npy"] + argv)
        assert status == 1 and text in err and len(stdout.splitlines()) == 13, argv
    status, _, err = _deltae(capsys, [d / "a.npy", d / "b.npy", "--max-de", "200", "--max-mean", "200", "--max-p95", "200"])
    assert status == 0 and "frame 5:" not in err


def test_command_output_does_not_depend_on_batch_and_depth(capsys, tmp_path):
    """The shared device loop (pairs.stream_pairs): the maps and the CSV are the same bytes however the nine frames are cut into
    batches and spread over buffer sets -- one set, three sets, a batch per frame, the whole clip in one batch."""
    got = []
    for batch, depth in ((8, 2), (1, 1), (3, 3), (9, 1)):
        out, csv = tmp_path / f"o_{batch}_{depth}.npy", tmp_path / f"w_{batch}_{depth}.csv"
        status, stdout, err = _deltae(capsys, ["synthetic:64x48:9:noise", "synthetic:64x48:9:structured", out, "--csv", csv, "--batch", batch, "--depth", depth])
        assert status == 0 and stdout == "" and "deltae: 9 frames" in err
        got.append((out.read_bytes(), csv.read_bytes()))
    assert np.load(tmp_path / "o_8_2.npy").shape == (9, 48, 64, 3) and np.load(tmp_path / "o_8_2.npy").any()
    assert len(got[0][1].splitlines()) == 10
    for other in got[1:]:
        assert other == got[0]
