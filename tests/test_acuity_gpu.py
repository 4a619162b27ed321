"""GPU: the receptor-noise-limited distance behind the observer's acuity blur (csrc/receptor_acuity.hip) against the
float64 definition of tests/_acuity_ref.py, and `deltae --acuity` end to end.  The shapes are the smallest at which a 64 x 32 tile with a
halo of up to 16 can go wrong, not the workload's: at 1 x 1 every tap folds to one pixel; 2 x 3 reflects many times; 5 x 7 is smaller
than every radius but the smallest; 16 x 16 is below one tile; 33 x 70 is a tile and a sliver in both directions; 48 x 96 has two tiles
across; 70 x 530 has 3 x 9 tiles with a partial last row and column, and tiles in the middle of its rows whose region needs no
folding at the small radii; 96 x 160 has one such tile at the largest radius.  Sigmas 0.2, 0.7, 1.0, 3.5 (Dog), 4.0 (the cap): 3, 7, 9, 29 and 33 taps (_acuity_ref.CASES says which size
runs which).  Observers: test_receptor_gpu.py's three.  Frames: that file's five kinds and a spark (_acuity_ref.frames).

Accuracy.  The device's float32 dS of every pixel is held to _acuity_ref.BOUND = 2e-4 absolute against the float64 yardstick: 8 x the
largest |float32 restatement of the definition - yardstick| over these very frames, which test_acuity_host.py measures on the CPU
(2.35e-5, kept as F32_FIGURE = 2.5e-5); the factor 8 is test_receptor_gpu.py's, because the device's logf and division round
differently from NumPy's.  Measured on an MI355X on the frames of this file, the largest |device - yardstick| is 2.34e-5 (Dog, the ramp
at 70 x 530, sigma 1.0; the four-class observer's largest is 1.66e-5, HoneyBee's 8.1e-6); per size: DEVICE_FIGURES below.

Everything else has no tolerance: a pixel whose reflected neighbourhood is the same in A and B is exactly 0, greys are exactly 0 apart,
the record (the float64 sum in the kernel's own order included) and the map follow from the device's own float32 values, and a frame's
bytes do not depend on its batch or on the alignment of its buffers."""
import numpy as np
import pytest

import _acuity_ref as A
import _deltae_ref as E
from animal_vision_amd.metrics import species_acuity as _feature  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu

# the largest |device - yardstick| per observer and per size, as test_values_against_the_float64_definition prints them on an MI355X
DEVICE_FIGURES = """Dog 2.34e-5 (the ramp at 70 x 530, sigma 1.0), the four-class observer 1.66e-5 (the ramp at 70 x 530, sigma 3.5),
HoneyBee 8.1e-6 (the ramp at 70 x 530, sigma 1.0); by size: 1 x 1 7.4e-6, 2 x 3 1.05e-5, 5 x 7 1.20e-5, 16 x 16 1.06e-5, 33 x 70 1.60e-5,
48 x 96 1.72e-5, 70 x 530 2.34e-5, 96 x 160 2.01e-5.  Two flat frames: within 5.0e-6 of the per-pixel distance.  The checkerboard, Dog:
1.5037 per pixel, 0.0430 behind acuity 3.5 px."""

SIZES = list(A.CASES)
TILE_W, TILE_H, THREADS = 64, 32, 256
_want = {}


def _observers():
    from animal_vision_amd.metrics import Observer, observer_for

    return [observer_for("Dog", (0.05, 0.05)), observer_for("HoneyBee", (0.13, 0.06, 0.12)), Observer("four", A.FOUR, (0.08,) * 4)]


def _yardstick(H, W, obs, sigma):
    key = (H, W, obs.name, sigma)
    if key not in _want:
        a, b = A.frames(H, W)
        want = A.delta_s(a, b, obs.matrix, obs.weber, obs.floor, sigma)
        want.setflags(write=False)
        _want[key] = want
    return _want[key]


def _fold(s):
    """s[:, :n] -> the sum a tree of halvings leaves in element 0 of every row: what lane 0 of a wave holds after the __shfl_down steps,
    and thread 0 after tile_partials_sum's tree."""
    s = s.copy()
    o = s.shape[1] // 2
    while o > 0:
        s[:, :o] = s[:, :o] + s[:, o : 2 * o]
        o //= 2
    return s[:, 0]


def _kernel_sum(v):
    """The float64 sum of a frame's float32 values in the kernel's order: a 64 x 32 tile per workgroup, tiles in raster order; thread
    (segment t >> 6, column t & 63) adds its eight pixels, rows 8 segment ... + 7 of the column, from the top down (pixels outside the
    frame add nothing); a wave -- one segment -- folds its 64 lanes by halves; the four waves are added in order; thread t of the final
    kernel adds partials t, t + 256, ... and the 256 threads are folded by halves."""
    H, W = v.shape
    ty, tx = -(-H // TILE_H), -(-W // TILE_W)
    pad = np.zeros((ty * TILE_H, tx * TILE_W))  # adding 0.0 is exact
    pad[:H, :W] = v.astype(np.float64)
    partials = np.zeros(-(-(ty * tx) // THREADS) * THREADS)
    for j in range(ty):
        for i in range(tx):
            t = pad[j * TILE_H : (j + 1) * TILE_H, i * TILE_W : (i + 1) * TILE_W].reshape(4, 8, TILE_W)  # segment, row of it, column
            s = np.zeros((4, TILE_W))
            for o in range(8):
                s = s + t[:, o, :]
            w = _fold(s)
            partials[j * tx + i] = ((w[0] + w[1]) + w[2]) + w[3]
    t = np.zeros(THREADS)
    for r in partials.reshape(-1, THREADS):
        t = t + r
    return float(_fold(t.reshape(1, THREADS))[0])


def _check_record(rec, v, T, what):
    want = E.record(v, T)
    assert np.array_equal(rec.hist, want["hist"]), what
    assert (np.float32(rec.max_de).tobytes(), rec.max_x, rec.max_y) == (np.float32(want["max_de"]).tobytes(), want["max_x"], want["max_y"]), what
    assert rec.beyond == want["beyond"], what
    assert np.float64(rec.sum).tobytes() == np.float64(_kernel_sum(v)).tobytes(), (what, rec.sum, _kernel_sum(v))
    assert rec.pixels == v.size and rec.mean == rec.sum / v.size
    for q in (0.5, 0.95, 1.0):
        assert rec.percentile(q) == E.percentile(want["hist"], want["max_de"], q), (what, q)


def _zero_record(r, n):
    return r.hist[0] == n and r.hist.sum() == n and (r.sum, r.max_de, r.max_x, r.max_y, r.beyond) == (0.0, 0.0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("H,W", SIZES)
def test_values_against_the_float64_definition(H, W):
    from animal_vision_amd.metrics import receptor_delta_values

    a, b = A.frames(H, W)
    for sigma in A.CASES[(H, W)]:
        for obs in _observers():
            want = _yardstick(H, W, obs, sigma)
            got = receptor_delta_values(a, b, obs, acuity=sigma)
            assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and (got >= 0).all()
            dev = np.abs(got.astype(np.float64) - want).reshape(len(A.KINDS), -1).max(axis=1)
            print(f"acuity {H}x{W} sigma {sigma} {obs.name}: largest |device - yardstick| {dev.max():.3e} ("
                  + ", ".join(f"{k} {d:.2e}" for k, d in zip(A.KINDS, dev)) + f"), largest dS {want.max():.4f}")
            for i, name in enumerate(A.KINDS):
                assert dev[i] <= A.BOUND, (obs.name, name, H, W, sigma, float(dev[i]))
            if H * W >= 64:
                assert got[0].max() > 0.5 and got[2].max() > 0 and got[5].max() > 0  # the pairs do differ, also behind the blur
            one = receptor_delta_values(a[2], b[2], obs, acuity=sigma)  # one frame: H x W
            assert one.shape == (H, W) and one.tobytes() == got[2].tobytes()


# ------------------------------------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("sigma", [3.5, 0.2])
def test_one_changed_pixel_is_seen_in_its_neighbourhood_only(sigma):
    """B is A with one pixel changed: exactly 0 wherever the reflected (2R + 1)^2 neighbourhood excludes it -- a wrong halo, a wrong
    fold or a dependence on the tile order shows here."""
    from animal_vision_amd.metrics import receptor_delta_values

    H, W = 70, 530
    a = A.frames(H, W)[0][0]
    R = (A.ksize(sigma) - 1) // 2
    # an interior pixel, both sides of the vertical seam x = 63 | 64 and of the horizontal seam y = 31 | 32, a corner, the last pixel
    spots = [(45, 300), (10, 63), (10, 64), (31, 200), (32, 200), (31, 63), (32, 64), (0, 0), (H - 1, W - 1)]
    b = np.stack([a] * len(spots))
    for i, (y, x) in enumerate(spots):
        b[i, y, x] ^= 0x55
    for obs in _observers():
        v = receptor_delta_values(np.stack([a] * len(spots)), b, obs, acuity=sigma)
        for i, (y, x) in enumerate(spots):
            near = A.near_mask(H, W, y, x, R)
            assert near[y, x] and v[i, y, x] > 0, (obs.name, y, x)
            assert not v[i][~near].any(), (obs.name, y, x, int((v[i][~near] != 0).sum()))


@pytest.mark.parametrize("H,W", [(5, 7), (70, 530)])
def test_greys_are_exactly_zero_apart(H, W):
    from animal_vision_amd.metrics import receptor_delta_map, receptor_delta_values

    g1, g2 = A.grey_frames(H, W)
    for obs in _observers():
        for sigma in (1.0, 4.0):
            v = receptor_delta_values(g1, g2, obs, acuity=sigma)
            assert v.dtype == np.float32 and not v.any(), (obs.name, sigma, float(v.max()))
            plain, rec = receptor_delta_map(g1, g2, obs, mode="plain", gain=255.0, threshold=0.0, acuity=sigma)
            assert not plain.any() and _zero_record(rec, H * W), (obs.name, sigma)


@pytest.mark.parametrize("H,W", SIZES)
def test_identical_frames_give_a_zero_record_and_a_black_map(H, W):
    from animal_vision_amd.metrics import receptor_delta_map, receptor_delta_values

    a, _ = A.frames(H, W)
    for obs in _observers():
        for sigma in (A.CASES[(H, W)][0], A.CASES[(H, W)][-1]):
            v = receptor_delta_values(a, a.copy(), obs, acuity=sigma)
            assert v.dtype == np.float32 and not v.any(), (obs.name, sigma)
            plain, recs = receptor_delta_map(a, a.copy(), obs, mode="plain", gain=255.0, threshold=0.0, acuity=sigma)
            assert not plain.any() and all(_zero_record(r, H * W) for r in recs), (obs.name, sigma)


# ------------------------------------------------------------------------------------------------ the record and the map: no tolerance
@pytest.mark.parametrize("H,W", [(48, 96), (70, 530)])
def test_record_and_map_follow_the_devices_own_values(H, W):
    from animal_vision_amd.metrics import receptor_delta, receptor_delta_map, receptor_delta_values

    a, b = A.frames(H, W)
    sigma = A.CASES[(H, W)][-1]
    for obs in _observers():
        v = receptor_delta_values(a, b, obs, acuity=sigma)
        for mode, layout, G, T in (("heat", "map", None, 1.0), ("heat", "side", 10.0, 1.0), ("plain", "map", 10.0, 1.0), ("plain", "side", 2.5, 0.0),
                                   ("heat", "map", 255.0, 0.0), ("heat", "side", 0.37, 2.3)):
            got, recs = receptor_delta_map(a, b, obs, mode=mode, gain=G, threshold=T, layout=layout, acuity=sigma)
            assert got.dtype == np.uint8 and got.shape == (len(a), H, W * (3 if layout == "side" else 1), 3)
            only = receptor_delta(a, b, obs, T, acuity=sigma)
            for i, name in enumerate(A.KINDS):
                what = (obs.name, name, mode, layout, G, T, H, W)
                m = E.de_map(v[i], a[i], 10.0 if G is None else G, T, mode)  # the dim grey is the unfiltered A's
                assert np.array_equal(got[i], E.side(a[i], b[i], m) if layout == "side" else m), what  # and so are the panels
                _check_record(recs[i], v[i], T, what)
                assert only[i] == recs[i], what  # records only (no map) is the same record
        one, rec = receptor_delta_map(a[0], b[0], obs, acuity=sigma)  # one frame, every default: heat, G = 10, T = 1, the map alone
        assert np.array_equal(one, E.de_map(v[0], a[0], 10.0, 1.0, "heat")) and rec == receptor_delta(a[0], b[0], obs, acuity=sigma)


# ------------------------------------------------------------------------------------------------ batches and alignment
def test_a_frame_is_bit_equal_alone_in_a_batch_and_from_offset_buffers():
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, delta_e_records_from_bytes, receptor_delta_launch, receptor_delta_map, receptor_delta_values
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 48, 96
    a, b = A.frames(H, W)
    fb = H * W * 3
    d_a, d_b, d_o, d_r, d_v = ctx.malloc(fb + 32), ctx.malloc(fb + 32), ctx.malloc(3 * fb + 32), ctx.malloc(DELTA_E_RECORD_BYTES), ctx.malloc(H * W * 4)
    try:
        for obs, sigma in zip(_observers(), (3.5, 1.0, 4.0)):
            k = 2
            alone_map, alone_rec = receptor_delta_map(a[k], b[k], obs, layout="side", acuity=sigma)
            alone_v = receptor_delta_values(a[k], b[k], obs, acuity=sigma)
            assert alone_v.any()
            for place in range(5):  # at every place of a batch of five
                order = [(k + 1 + j) % 5 for j in range(4)]
                order.insert(place, k)
                got, recs = receptor_delta_map(a[order], b[order], obs, layout="side", acuity=sigma)
                assert np.array_equal(got[place], alone_map) and recs[place] == alone_rec, (obs.name, place)
                assert receptor_delta_values(a[order], b[order], obs, acuity=sigma)[place].tobytes() == alone_v.tobytes(), (obs.name, place)
            order = [(j * 5 + 1) % 6 for j in range(16)]  # a batch of 16: one launch
            got, recs = receptor_delta_map(a[order], b[order], obs, layout="side", acuity=sigma)
            for j in (i for i, o in enumerate(order) if o == k):
                assert np.array_equal(got[j], alone_map) and recs[j] == alone_rec, (obs.name, j)
            assert any(o == k for o in order)
            # from buffers offset by one byte
            for off_a, off_b, off_o in ((1, 1, 1), (1, 0, 0), (0, 0, 1)):
                va, vb, vo = d_a.view(off_a, fb), d_b.view(off_b, fb), d_o.view(off_o, 3 * fb)
                ctx.upload(a[k], va)
                ctx.upload(b[k], vb)
                receptor_delta_launch(ctx, va, vb, 1, H, W, vo, d_r, observer=obs, layout="side", d_float=d_v, acuity=sigma)
                got = ctx.download(vo, (H, 3 * W, 3), np.uint8)
                rec = delta_e_records_from_bytes(ctx.download(d_r, (DELTA_E_RECORD_BYTES,), np.uint8), 1)[0]
                val = ctx.download(d_v, (H, W), np.float32)
                assert np.array_equal(got, alone_map) and rec == alone_rec and val.tobytes() == alone_v.tobytes(), (obs.name, off_a, off_b, off_o)
    finally:
        for d in (d_a, d_b, d_o, d_r, d_v):
            d.free()


# ------------------------------------------------------------------------------------------------ the plain distance
def test_flat_frames_and_the_checkerboard_against_the_plain_distance():
    """A flat frame blurs to itself (the taps sum to 1 within float32 rounding), so the acuity value of two flat frames is the plain
    value within the bound; a one-pixel checkerboard against its mean colour is tens of times closer behind Dog's blur than per pixel."""
    from animal_vision_amd.metrics import receptor_delta, receptor_delta_values

    H, W = 33, 70
    colours = [((200, 60, 60), (60, 200, 60)), ((10, 10, 40), (12, 9, 40)), ((255, 255, 0), (0, 0, 255)), ((128, 128, 128), (90, 140, 128))]
    a = np.stack([np.broadcast_to(np.array(c, np.uint8), (H, W, 3)) for c, _ in colours])
    b = np.stack([np.broadcast_to(np.array(c, np.uint8), (H, W, 3)) for _, c in colours])
    for obs in _observers():
        plain = receptor_delta_values(a, b, obs)
        assert plain.min() > 0
        for sigma in (0.7, 3.5):
            v = receptor_delta_values(a, b, obs, acuity=sigma)
            d = float(np.abs(v.astype(np.float64) - plain.astype(np.float64)).max())
            print(f"acuity flat frames {obs.name} sigma {sigma}: largest |acuity - plain| {d:.3e}")
            assert d <= A.BOUND, (obs.name, sigma, d)
    board, flat = A.checkerboard()
    dog = _observers()[0]
    per_pixel, seen = receptor_delta(board, flat, dog), receptor_delta(board, flat, dog, acuity=3.5)
    print(f"checkerboard 64x64, Dog (0.05, 0.05): mean dS per pixel {per_pixel.mean:.4f} (largest {per_pixel.max_de:.4f}), behind acuity 3.5 px "
          f"{seen.mean:.4f} (largest {seen.max_de:.4f})")
    assert per_pixel.mean > 1 and seen.mean < per_pixel.mean / 10


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing():
    import ctypes

    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, observer_for
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 16, 16
    fb = H * W * 3
    d_in = ctx.upload(np.zeros(3 * fb, np.uint8))
    a, b = d_in.ptr, d_in.ptr + fb
    d_out = ctx.upload(np.full(3 * fb, 0xAB, np.uint8))
    d_rec = ctx.upload(np.full(DELTA_E_RECORD_BYTES + 8, 0xAB, np.uint8))
    o, r = d_out.ptr, d_rec.ptr
    fn = _lib.lib.avx_receptor_acuity_u8
    dog = observer_for("Dog", (0.05, 0.05))
    nan, inf = float("nan"), float("inf")

    def desc(**kw):
        d = dog.desc()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return ctypes.byref(d)

    good = desc()
    try:
        calls = [(a, b, 1, H, W, good, s, 0, 10.0, 1.0, 0, o, r, None) for s in (0.19, 4.07, nan, inf, -1.0, 0.0, 4.0000001)]
        calls += [(a, b, 1, H, W, d, 1.0, 0, 10.0, 1.0, 0, o, r, None)
                  for d in (None, desc(struct_size=140), desc(n_receptors=1), desc(n_receptors=5), desc(matrix=(1, -0.1)), desc(matrix=(4, nan)), desc(n_receptors=3),
                            desc(weber=(0, 0.009)), desc(weber=(1, nan)), desc(floor=0.0), desc(floor=0.2))]
        calls += [(None, b, 1, H, W, good, 1.0, 0, 10.0, 1.0, 0, o, r, None), (a, None, 1, H, W, good, 1.0, 0, 10.0, 1.0, 0, o, r, None),
                  (a, b, 1, H, W, good, 1.0, 0, 10.0, 1.0, 0, o, None, None), (a, b, 0, H, W, good, 1.0, 0, 10.0, 1.0, 0, o, r, None),
                  (a, b, 17, H, W, good, 1.0, 0, 10.0, 1.0, 0, o, r, None), (a, b, 1, 0, W, good, 1.0, 0, 10.0, 1.0, 0, o, r, None),
                  (a, b, 1, H, -1, good, 1.0, 0, 10.0, 1.0, 0, o, r, None), (a, b, 1, 1 << 16, 1 << 16, good, 1.0, 0, 10.0, 1.0, 0, o, r, None),
                  (a, b, 1, H, W, good, 1.0, 2, 10.0, 1.0, 0, o, r, None), (a, b, 1, H, W, good, 1.0, 0, 0.0, 1.0, 0, o, r, None),
                  (a, b, 1, H, W, good, 1.0, 0, 255.5, 1.0, 0, o, r, None), (a, b, 1, H, W, good, 1.0, 0, nan, 1.0, 0, o, r, None),
                  (a, b, 1, H, W, good, 1.0, 0, 10.0, -1.0, 0, o, r, None), (a, b, 1, H, W, good, 1.0, 0, 10.0, inf, 0, o, r, None),
                  (a, b, 1, H, W, good, 1.0, 0, 10.0, 1.0, 2, o, r, None), (a, b, 1, H, W, good, 1.0, 0, 10.0, 1.0, 0, o, r + 4, None),
                  (a, b, 1, H, W, good, 1.0, 0, 10.0, 1.0, 0, o, r, o + 2), (a, b, 1, H, W, good, 1.0, 0, 10.0, 1.0, 0, a, r, None),
                  (a, b, 1, H, W, good, 1.0, 0, 10.0, 1.0, 1, b - 10, r, None)]
        for args in calls:
            assert fn(ctx._h, *args, ctx.stream) == _lib.AVX_ERR_INVALID, args
            assert _lib.lib.avx_last_error(ctx._h).decode().startswith("avx_receptor_acuity_u8:"), (args, _lib.lib.avx_last_error(ctx._h))
        ctx.sync()
        assert (ctx.download(d_out, (3 * fb,), np.uint8) == 0xAB).all() and (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8) == 0xAB).all()
        for s in (0.2, 4.0):  # the ends are good calls: black against black
            assert fn(ctx._h, a, b, 1, H, W, good, s, 1, 2.0, 1.0, 0, o, r, None, ctx.stream) == 0
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


def test_command_with_an_acuity(capsys, tmp_path):
    from animal_vision_amd.metrics import observer_for, receptor_delta, receptor_delta_map
    from animal_vision_amd.pairs import num

    a, b = A.frames(48, 96)
    pa, pb, csv, out = tmp_path / "a.npy", tmp_path / "b.npy", tmp_path / "f.csv", tmp_path / "o.npy"
    np.save(pa, a)
    np.save(pb, b)
    dog = observer_for("Dog", (0.05, 0.05))
    base = [pa, pb, "--observer", "Dog", "--weber", "0.05,0.05"]
    recs = receptor_delta(a, b, dog, acuity=3.5)
    status, stdout, err = _deltae(capsys, base + ["--acuity", "species", "--csv", csv])
    assert status == 0 and stdout == "" and csv.read_text() == _rows(recs)
    assert f"deltae: 6 frames, mean RNL dS (Dog, weber 0.05,0.05, floor 0.001, acuity 3.5 px) {num(sum(r.mean for r in recs) / 6)}, largest dS " in err
    want, recs = receptor_delta_map(a, b, dog, acuity=3.5)
    seen = []
    for batch in ("1", "4"):
        status, stdout, err = _deltae(capsys, [pa, pb, out] + base[2:] + ["--acuity", "3.5", "--csv", csv, "--batch", batch])
        assert status == 0 and stdout == "" and np.array_equal(np.load(out), want) and csv.read_text() == _rows(recs), batch
        assert "acuity 3.5 px" in err
        seen.append((out.read_bytes(), csv.read_bytes()))
    assert seen[0] == seen[1]
    want, recs = receptor_delta_map(a, b, dog, mode="plain", gain=4, layout="side", threshold=0.5, acuity=1.0)
    status, _, err = _deltae(capsys, [pa, pb, out] + base[2:] + ["--acuity", "1", "--mode", "plain", "--gain", "4", "--layout", "side", "--threshold", "0.5", "--csv", csv])
    assert status == 0 and np.array_equal(np.load(out), want) and csv.read_text() == _rows(recs) and "acuity 1 px" in err
    # without --acuity the command is what it was: the per-pixel distance
    plain = receptor_delta(a, b, dog)
    status, stdout, err = _deltae(capsys, base)
    assert status == 0 and stdout == _rows(plain) and "acuity" not in err and "RNL dS (Dog, weber 0.05,0.05, floor 0.001) " in err
    assert plain != receptor_delta(a, b, dog, acuity=3.5)
