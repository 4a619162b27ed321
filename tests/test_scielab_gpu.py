"""GPU: the S-CIELAB kernels (csrc/scielab.hip) against the float64 definition of tests/_scielab_ref.py, and
`deltae --ppd` end to end.  The shapes are the smallest at which the kernels can go wrong, not the workload's.  The row kernel's tile is
256 x 4 pixels and the column kernel's 64 x 32: 1 x 1; 5 x 7 is below every support; 33 x 50 is odd and its planes are stored value by
value; 64 x 96 has W a multiple of 4 (16-byte plane stores); 70 x 530 is ragged and spans three tiles of either kernel in each
direction (seams); 3 x 300 is shorter than the halo of any ppd above 4.  ppd 2 (R = 1), 9, 22.5 (not an integer), 60 and 128 (R = 64)
are each run on at least two shapes.  Frames: noise, a dark frame (codes 0 .. 23: the linear branch of f), a smooth ramp and saturated
primaries (the filters leave negative t next to their edges); B is A with +-3 noise, or with a region replaced.

Accuracy.  The device's float32 dE of every pixel is held to BOUND = 1e-3, the bound `deltae` is held to, against the float64 yardstick.
Measured on an MI355X on the frames of this file: the largest |device - yardstick| is 1.41e-4 (noise at 70 x 530, ppd 128; 1.30e-4 at
ppd 60 and 1.10e-4 at 22.5 there, 1.20e-4 at 64 x 96 ppd 60, 1.02e-4 at 33 x 50, 9.7e-5 at 3 x 300, 4.4e-5 at 5 x 7, 1.1e-5 at 1 x 1; by
frame: noise 1.41e-4, ramp and primaries 1.08e-4, dark 2.8e-5).

Everything else has no tolerance: the record and the map follow from the device's own float32 values as in tests/test_deltae_gpu.py,
a frame's bytes do not depend on its batch, and equal neighbourhoods give exactly 0."""
import numpy as np
import pytest

import _deltae_ref as E
import _scielab_ref as S
from animal_vision_amd.metrics import scielab_launch as _feature  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu

BOUND = 1e-3
CASES = [(1, 1, 2), (1, 1, 128), (5, 7, 9), (5, 7, 60), (33, 50, 2), (33, 50, 22.5), (33, 50, 128), (64, 96, 9), (64, 96, 60), (70, 530, 22.5),
         (70, 530, 60), (70, 530, 128), (3, 300, 9), (3, 300, 128)]
ONE_PPD_PER_SHAPE = [(1, 1, 128), (5, 7, 60), (33, 50, 22.5), (64, 96, 9), (70, 530, 60), (3, 300, 128)]
KINDS = ("noise", "dark", "ramp", "primaries")
_pairs, _want = {}, {}


def _frames(H, W):
    """The four frame pairs of a size as two stacks; computed once, read-only."""
    if (H, W) not in _pairs:
        seed = H * 1000 + W
        a = np.stack([S.frame(k, H, W, seed + i) for i, k in enumerate(KINDS)])
        b = np.stack([S.jitter(x, seed + 10 + i) for i, x in enumerate(a)])
        b[2] = a[2]
        b[2, H // 3 : H // 3 + max(1, H // 4), W // 5 : W // 5 + max(1, W // 3)] = S.frame("noise", max(1, H // 4), max(1, W // 3), seed + 20)  # a region replaced
        a.setflags(write=False), b.setflags(write=False)
        _pairs[(H, W)] = (a, b)
    return _pairs[(H, W)]


def _yardstick(H, W, ppd):
    if (H, W, ppd) not in _want:
        a, b = _frames(H, W)
        want = np.stack([S.scielab(x, y, ppd) for x, y in zip(a, b)])
        want.setflags(write=False)
        _want[(H, W, ppd)] = want
    return _want[(H, W, ppd)]


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
@pytest.mark.parametrize("H,W,ppd", CASES)
def test_values_against_the_float64_definition(H, W, ppd):
    from animal_vision_amd.metrics import scielab_values

    a, b = _frames(H, W)
    want = _yardstick(H, W, ppd)
    got = scielab_values(a, b, ppd=ppd)
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and (got >= 0).all()
    dev = np.abs(got.astype(np.float64) - want)
    for i, name in enumerate(KINDS):
        print(f"scielab {H}x{W} ppd {ppd:g} {name}: largest |device - yardstick| {dev[i].max():.3e}, largest dE {want[i].max():.4f}, mean dE {want[i].mean():.4f}")
    for i, name in enumerate(KINDS):
        assert dev[i].max() <= BOUND, (name, H, W, ppd, float(dev[i].max()))
    one = scielab_values(a[1], b[1], ppd=ppd)  # one frame: H x W
    assert one.shape == (H, W) and one.tobytes() == got[1].tobytes()


def test_the_checkerboard_no_viewer_resolves():
    from animal_vision_amd.metrics import delta_e, scielab, scielab_values

    a, b = S.checkerboard()
    plain, r60, r30 = delta_e(a, b), scielab(a, b, ppd=60), scielab(a, b, ppd=30)
    assert 11.8 < plain.mean < 11.85 and r60.mean < 0.25 * plain.mean and abs(r60.mean - S.scielab(a, b, 60).mean()) <= BOUND
    assert abs(r30.mean - S.scielab(a, b, 30).mean()) <= BOUND and 5.0 < r30.mean < 5.25
    assert scielab_values(a, b, ppd=60)[30:-30, 30:-30].max() < 0.05


# ------------------------------------------------------------------------------------------------ the record and the map: no tolerance
@pytest.mark.parametrize("H,W,ppd", ONE_PPD_PER_SHAPE)
def test_record_and_map_follow_the_devices_own_values(H, W, ppd):
    from animal_vision_amd.metrics import scielab, scielab_map, scielab_values

    a, b = _frames(H, W)
    v = scielab_values(a, b, ppd=ppd)
    for mode, layout, G, T in (("heat", "map", None, 1.0), ("heat", "side", 10.0, 1.0), ("plain", "map", 10.0, 1.0), ("plain", "side", 2.5, 0.0),
                               ("heat", "map", 255.0, 0.0), ("heat", "side", 0.37, 2.3)):
        got, recs = scielab_map(a, b, ppd=ppd, mode=mode, gain=G, threshold=T, layout=layout)
        assert got.dtype == np.uint8 and got.shape == (len(a), H, W * (3 if layout == "side" else 1), 3)
        only = scielab(a, b, ppd=ppd, threshold=T)
        for i, name in enumerate(KINDS):
            what = (name, mode, layout, G, T, H, W, ppd)
            m = E.de_map(v[i], a[i], 10.0 if G is None else G, T, mode)  # the dim grey is the unfiltered A's
            assert np.array_equal(got[i], E.side(a[i], b[i], m) if layout == "side" else m), what  # the panels are the unfiltered A and B
            _check_record(recs[i], v[i], T, what)
            assert only[i] == recs[i], what  # records only (no map) is the same record
    one, rec = scielab_map(a[0], b[0], ppd=ppd)  # one frame, every default: heat, G = 10, T = 1, the map alone
    assert np.array_equal(one, E.de_map(v[0], a[0], 10.0, 1.0, "heat")) and rec == scielab(a[0], b[0], ppd=ppd)


# ------------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("H,W,ppd", [(33, 50, 9), (70, 530, 22.5)])
def test_a_frame_is_bit_equal_in_any_batch_and_at_any_place(H, W, ppd):
    from animal_vision_amd.metrics import scielab_map, scielab_values

    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (16, H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    m1, r1 = scielab_map(a[0], b[0], ppd=ppd, layout="side")  # batch 1
    v1 = scielab_values(a[0], b[0], ppd=ppd)
    for slot in (0, 2, 15):
        aa, bb = np.roll(a, slot, axis=0), np.roll(b, slot, axis=0)
        got, recs = scielab_map(aa, bb, ppd=ppd, layout="side")
        assert np.array_equal(got[slot], m1) and recs[slot] == r1, slot
        assert scielab_values(aa, bb, ppd=ppd)[slot].tobytes() == v1.tobytes(), slot
    whole, recs = scielab_map(a, b, ppd=ppd, layout="side")
    vals = scielab_values(a, b, ppd=ppd)
    for lo in (0, 8):  # the 16 in two halves
        half, hrecs = scielab_map(a[lo : lo + 8], b[lo : lo + 8], ppd=ppd, layout="side")
        assert np.array_equal(half, whole[lo : lo + 8]) and hrecs == recs[lo : lo + 8]
        assert scielab_values(a[lo : lo + 8], b[lo : lo + 8], ppd=ppd).tobytes() == vals[lo : lo + 8].tobytes()
    again, recs2 = scielab_map(a, b, ppd=ppd, layout="side")
    assert np.array_equal(again, whole) and recs2 == recs  # and repeatable


@pytest.mark.parametrize("off", [1, 4])
def test_offset_buffers_give_the_same_bytes(off):
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, delta_e_records_from_bytes, scielab_launch, scielab_map, scielab_values
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W, ppd = 64, 96, 9
    a, b = _frames(H, W)
    n, fb = len(a), H * W * 3
    v0 = scielab_values(a, b, ppd=ppd)
    d_a, d_b, d_o, d_r, d_v = ctx.malloc(n * fb + 32), ctx.malloc(n * fb + 32), ctx.malloc(3 * n * fb + 32), ctx.malloc(n * DELTA_E_RECORD_BYTES), ctx.malloc(n * H * W * 4)
    try:
        for off_a, off_b, off_o in ((off, off, off), (off, 0, 0), (0, 0, off)):
            va, vb = d_a.view(off_a, n * fb), d_b.view(off_b, n * fb)
            ctx.upload(a, va)
            ctx.upload(b, vb)
            for mode, layout in (("heat", "map"), ("plain", "side")):
                wide = 3 if layout == "side" else 1
                vo = d_o.view(off_o, wide * n * fb)
                scielab_launch(ctx, va, vb, n, H, W, vo, d_r, ppd=ppd, mode=mode, layout=layout, d_float=d_v)
                got = ctx.download(vo, (n, H, W * wide, 3), np.uint8)
                recs = delta_e_records_from_bytes(ctx.download(d_r, (n * DELTA_E_RECORD_BYTES,), np.uint8), n)
                v = ctx.download(d_v, (n, H, W), np.float32)
                assert v.tobytes() == v0.tobytes(), (off_a, off_b, off_o)
                ref_map, ref_recs = scielab_map(a, b, ppd=ppd, mode=mode, layout=layout)
                assert np.array_equal(got, ref_map) and recs == ref_recs, (mode, layout, off_a, off_b, off_o)
    finally:
        for d in (d_a, d_b, d_o, d_r, d_v):
            d.free()


# ------------------------------------------------------------------------------------------------ exact zeros
@pytest.mark.parametrize("H,W,ppd", ONE_PPD_PER_SHAPE)
def test_identical_frames_are_exactly_zero(H, W, ppd):
    from animal_vision_amd.metrics import scielab_map, scielab_values

    a, _ = _frames(H, W)
    v = scielab_values(a, a.copy(), ppd=ppd)
    assert not v.any() and v.dtype == np.float32
    plain, recs = scielab_map(a, a.copy(), ppd=ppd, mode="plain", gain=255.0, threshold=0.0)
    assert not plain.any()
    for r in recs:
        assert r.hist[0] == H * W and r.hist.sum() == H * W and (r.sum, r.max_de, r.max_x, r.max_y, r.beyond) == (0.0, 0.0, 0, 0, 0)


@pytest.mark.parametrize("H,W,ppd", [(64, 96, 9), (70, 530, 22.5), (70, 530, 2), (33, 50, 22.5)])
def test_a_change_reaches_exactly_its_support(H, W, ppd):
    from animal_vision_amd.metrics import scielab_values

    R = S.radius(ppd)
    for kind in ("noise", "primaries"):
        a = S.frame(kind, H, W, 77)
        b = a.copy()
        y0, y1, x0, x1 = H // 2 - 4, H // 2 - 1, W // 2 - 10, W // 2 - 5  # 70 x 530: rows 31 .. 33, columns 255 .. 259, across the seams of both kernels' tiles
        b[y0:y1, x0:x1] = 255 - b[y0:y1, x0:x1]
        v = scielab_values(a, b, ppd=ppd)
        near = np.zeros((H, W), bool)
        near[max(0, y0 - R) : y1 + R, max(0, x0 - R) : x1 + R] = True
        assert not v[~near].any(), (kind, int((v[~near] != 0).sum()))
        assert v[y0:y1, x0:x1].min() > 0 and v.max() > 1
        # the upper half identical, with R rows of margin
        c = a.copy()
        c[H // 2 :] = S.frame("noise", H - H // 2, W, 78)
        v = scielab_values(a, c, ppd=ppd)
        assert not v[: max(0, H // 2 - R)].any() and v[H // 2 :].max() > 1, kind
    # one flipped pixel: (2R + 1)^2 candidates, no more
    a = S.frame("noise", H, W, 79)
    b = a.copy()
    b[H // 2, W // 2] ^= 0x55
    v = scielab_values(a, b, ppd=ppd)
    hit = np.zeros((H, W), bool)
    hit[max(0, H // 2 - R) : H // 2 + R + 1, max(0, W // 2 - R) : W // 2 + R + 1] = True
    assert not v[~hit].any() and v[H // 2, W // 2] > 0


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_ppd_launches_nothing():
    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 16, 16
    fb = H * W * 3
    d_in = ctx.upload(np.zeros(3 * fb, np.uint8))
    a, b = d_in.ptr, d_in.ptr + fb
    d_out = ctx.upload(np.full(3 * fb, 0xAB, np.uint8))
    d_rec = ctx.upload(np.full(DELTA_E_RECORD_BYTES + 8, 0xAB, np.uint8))
    o, r = d_out.ptr, d_rec.ptr
    fn = _lib.lib.avx_scielab_u8
    nan, inf = float("nan"), float("inf")
    try:
        for args in ((a, b, 1, H, W, 1.9, 0, 10.0, 1.0, 0, o, r, None), (a, b, 1, H, W, 128.5, 0, 10.0, 1.0, 0, o, r, None), (a, b, 1, H, W, nan, 0, 10.0, 1.0, 0, o, r, None),
                     (a, b, 1, H, W, inf, 0, 10.0, 1.0, 0, o, r, None), (a, b, 1, H, W, 0.0, 0, 10.0, 1.0, 0, o, r, None), (a, b, 1, H, W, -60.0, 0, 10.0, 1.0, 0, o, r, None),
                     (None, b, 1, H, W, 60.0, 0, 10.0, 1.0, 0, o, r, None), (a, b, 17, H, W, 60.0, 0, 10.0, 1.0, 0, o, r, None), (a, b, 1, 0, W, 60.0, 0, 10.0, 1.0, 0, o, r, None),
                     (a, b, 1, H, W, 60.0, 2, 10.0, 1.0, 0, o, r, None), (a, b, 1, H, W, 60.0, 0, 0.0, 1.0, 0, o, r, None), (a, b, 1, H, W, 60.0, 0, 10.0, -1.0, 0, o, r, None),
                     (a, b, 1, H, W, 60.0, 0, 10.0, 1.0, 2, o, r, None), (a, b, 1, H, W, 60.0, 0, 10.0, 1.0, 0, o, r + 4, None), (a, b, 1, H, W, 60.0, 0, 10.0, 1.0, 0, a, r, None)):
            assert fn(ctx._h, *args, ctx.stream) == _lib.AVX_ERR_INVALID, args
            assert _lib.lib.avx_last_error(ctx._h).decode().startswith("avx_scielab_u8:"), args
        ctx.sync()
        assert (ctx.download(d_out, (3 * fb,), np.uint8) == 0xAB).all() and (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8) == 0xAB).all()
        assert fn(ctx._h, a, b, 1, H, W, 60.0, 1, 2.0, 1.0, 0, o, r, None, ctx.stream) == 0  # the good call still works: black against black
        ctx.sync()
        assert not ctx.download(d_out, (fb,), np.uint8).any() and (ctx.download(d_out, (3 * fb,), np.uint8)[fb:] == 0xAB).all()
        assert (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8)[DELTA_E_RECORD_BYTES:] == 0xAB).all()  # nothing behind the record
    finally:
        for d in (d_in, d_out, d_rec):
            d.free()


# ------------------------------------------------------------------------------------------------ the command
def _deltae(capsys, argv):
    from animal_vision_amd import deltae

    status = deltae.main([str(v) for v in argv])
    cap = capsys.readouterr()
    return status, cap.out, cap.err


def _rows(recs):
    from animal_vision_amd.deltae import CSV_HEADER, format_row

    return CSV_HEADER + "\n" + "".join(format_row(i, r) + "\n" for i, r in enumerate(recs))


def _synthetic(spec, n):
    from animal_vision_amd.renderers import VideoRenderer

    vr = VideoRenderer(read_path=spec)
    vr.open()
    frames = np.stack([vr.get_image() for _ in range(n)])
    assert vr.get_image() is None
    vr.close()
    return frames


def test_command_with_and_without_ppd(capsys, tmp_path):
    from animal_vision_amd.metrics import delta_e, scielab, scielab_map
    from animal_vision_amd.pairs import num

    sa, sb = "synthetic:64x48:5:noise", "synthetic:64x48:5:structured"
    a, b = _synthetic(sa, 5), _synthetic(sb, 5)
    csv = tmp_path / "w.csv"
    status, stdout, err = _deltae(capsys, [sa, sb, "--ppd", "30", "--csv", csv])
    recs = scielab(a, b, ppd=30)
    assert status == 0 and stdout == "" and csv.read_text() == _rows(recs)
    assert f"deltae: 5 frames, mean S-CIELAB dE (ppd 30) {num(sum(r.mean for r in recs) / 5)}" in err
    status, stdout, _ = _deltae(capsys, [sa, sb, "--ppd", "30", "--batch", "2", "--threshold", "2.5"])
    assert status == 0 and stdout == _rows(scielab(a, b, ppd=30, threshold=2.5))
    for extra, kw in (([], {}), (["--mode", "plain", "--gain", "4", "--layout", "side", "--batch", "3", "--depth", "3"], dict(mode="plain", gain=4, layout="side"))):
        out = tmp_path / "o.npy"
        status, stdout, err = _deltae(capsys, [sa, sb, out, "--ppd", "30", "--csv", csv] + extra)
        want, recs = scielab_map(a, b, ppd=30, **kw)
        assert status == 0 and stdout == "" and np.array_equal(np.load(out), want) and csv.read_text() == _rows(recs), extra
    status, _, err = _deltae(capsys, [sa, sb, "--ppd", "30", "--max-mean", "0.01"])
    assert status == 1 and "deltae: frame 0: mean dE" in err
    # the default is unchanged: without --ppd the command is metrics.delta_e
    status, stdout, err = _deltae(capsys, [sa, sb])
    plain = delta_e(a, b)
    assert status == 0 and stdout == _rows(plain) and "mean dE " in err and "S-CIELAB" not in err
    assert plain != scielab(a, b, ppd=30)
