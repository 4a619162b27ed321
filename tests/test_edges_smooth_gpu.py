"""GPU: the edge-preserving smoothing in receptor space in front of the edges (csrc/receptor_smooth.hip) against the
float64 definition of tests/_smooth_ref.py, and `edges --smooth` end to end.  The shapes are the smallest at which a staged tile with
a halo, a rank that depends on the window and a walk in groups of frames can go wrong (_smooth_ref.CASES says which size runs which
setting, sigma and step): 1 x 1, 1 x 9, 2 x 3, 5 x 7, 16 x 16, 33 x 70, 70 x 130; (R, KEEP, ITER) = (1, 0.5, 2), (3, 0.3, 1),
(5, 0.33, 3), (2, 1.0, 1), (5, 0.01, 1); one test runs 16 frames of 1296 x 1296, the smallest batch that spans two scratch groups.

Exact, no tolerance: with iterations = 0 the planes route gives the fused kernel's values, map and record byte for byte (the float64
sum included: the back kernel keeps the fused kernel's blocks); a flat frame keeps its planes; a straight seam keeps them at
KEEP <= 0.5, on and off a tile seam; greys stay chromatically 0; a frame's outputs do not depend on its batch, its place, its scratch
group or its buffers' alignment; the record and the map follow from the device's own values.

Accuracy.  The device's float32 values, and its planes in the observer's metric, are held to _smooth_ref.BOUND = 1.2e-3 against the
float64 yardstick: 8 x the largest |float32 restatement - yardstick| over these very cases, which test_edges_smooth_host.py measures
on the CPU (1.343e-4, kept as F32_FIGURE = 1.5e-4; the values reach 86.4); no pixel is exempted.  DEVICE_FIGURES below is what
test_values_and_planes_against_the_float64_definition prints on an MI355X."""
import numpy as np
import pytest

import _acuity_ref as A
import _deltae_ref as DE
import _edges_ref as E
import _smooth_ref as S
from animal_vision_amd.metrics import receptor_smooth_planes as _feature  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu

DEVICE_FIGURES = """values: 1.105e-4 (the four-class observer, chromatic, the saturated frame at 33 x 70, (5, 0.33, 3), without blur, step 1); planes,
in the observer's metric: 1.078e-4 (Dog, achromatic, the saturated frame at 16 x 16, (5, 0.33, 3), without blur): below the float32 restatement's
own 1.343e-4 and an eleventh of the bound.  With one iteration the largest is 7.7e-5, at R = 1 and two iterations 5.0e-5."""

BLOCK_W, BLOCK_H = 64, 32


def _observers():
    from animal_vision_amd.metrics import Observer, observer_for

    return [observer_for("Dog", (0.05, 0.05)), observer_for("HoneyBee", (0.13, 0.06, 0.12)), Observer("four", A.FOUR, (0.08,) * 4)]


def _kw(obs, channel, sigma, D):
    return dict(achromatic=E.ACHROMATIC[obs.name], channel=channel, acuity=sigma or None, step=D)


def _all(f, obs, kw, smooth, mode="heat", gain=None, threshold=1.0, planes_of=None, offsets=(0, 0)):
    """One launch with every output: (maps, records, values, planes) of uint8 frames H x W x 3 or N <= 16 of them.  planes_of: download
    the planes of these frames only.  offsets: the input and the map start that many bytes into their buffers."""
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, delta_e_records_from_bytes, edges_planes, receptor_edges_launch
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    one = f.ndim == 3
    f = np.ascontiguousarray(f[None] if one else f)
    N, H, W = f.shape[:3]
    P = edges_planes(obs, kw["channel"])
    fb = N * H * W * 3
    bufs = [ctx.malloc(fb + 16), ctx.malloc(fb + 16), ctx.malloc(N * DELTA_E_RECORD_BYTES), ctx.malloc(N * H * W * 4), ctx.malloc(N * P * H * W * 4)]
    try:
        d_in, d_map, d_rec, d_val, d_pl = bufs
        d_in, d_map = d_in.view(offsets[0], fb), d_map.view(offsets[1], fb)
        ctx.upload(f, d_in)
        receptor_edges_launch(ctx, d_in, N, H, W, d_map, d_rec, observer=obs, mode=mode, gain=gain, threshold=threshold, d_float=d_val, smooth=smooth,
                              d_planes=d_pl, **kw)
        maps = ctx.download(d_map, (N, H, W, 3), np.uint8)
        recs = delta_e_records_from_bytes(ctx.download(d_rec, (N * DELTA_E_RECORD_BYTES,), np.uint8), N)
        vals = ctx.download(d_val, (N, H, W), np.float32)
        if planes_of is None:
            planes = ctx.download(d_pl, (N, P, H, W), np.float32)
        else:
            planes = np.stack([ctx.download(d_pl.view(i * P * H * W * 4, P * H * W * 4), (P, H, W), np.float32) for i in planes_of])
    finally:
        for b in bufs:
            b.free()
    return (maps[0], recs[0], vals[0], planes[0]) if one else (maps, recs, vals, planes)


def _zero_record(r, n):
    return r.hist[0] == n and r.hist.sum() == n and (r.sum, r.max_de, r.max_x, r.max_y, r.beyond) == (0.0, 0.0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ the anchor: iterations = 0
@pytest.mark.parametrize("H,W,runs", [(1, 1, ((0.0, 1), (4.0, 8))), (5, 7, ((0.0, 2), (3.5, 1))), (33, 70, ((0.0, 1), (0.2, 2), (3.5, 8))),
                                      (70, 530, ((0.0, 1), (3.5, 1), (4.0, 8)))])
def test_without_iterations_the_planes_route_is_the_fused_kernel_byte_for_byte(H, W, runs):
    from animal_vision_amd.metrics import receptor_edges, receptor_edges_map, receptor_edges_values

    assert all(r in E.CASES[(H, W)] for r in runs)
    f = E.frames(H, W)
    for sigma, D in runs:
        for k, obs in enumerate(_observers()):
            for ch in E.CHANNELS:
                kw = _kw(obs, ch, sigma, D)
                mode, G, T = (("heat", None, 1.0), ("plain", 2.5, 0.0), ("heat", 0.37, 2.3))[k]
                want_map, want_rec = receptor_edges_map(f, obs, mode=mode, gain=G, threshold=T, **kw)
                want_v = receptor_edges_values(f, obs, **kw)
                got_map, got_rec, got_v, planes = _all(f, obs, kw, (3, 0.5, 0), mode, G, T)
                what = (obs.name, ch, H, W, sigma, D)
                assert got_v.tobytes() == want_v.tobytes() and got_map.tobytes() == want_map.tobytes(), what
                for a, b in zip(got_rec, want_rec):
                    assert a == b and np.float64(a.sum).tobytes() == np.float64(b.sum).tobytes() and np.array_equal(a.hist, b.hist), what
                    assert (a.max_x, a.max_y, a.beyond, a.pixels) == (b.max_x, b.max_y, b.beyond, b.pixels), what
                # the keyword on the array entries takes the same route
                assert receptor_edges_values(f, obs, smooth=(1, 1.0, 0), **kw).tobytes() == want_v.tobytes(), what
                assert receptor_edges(f, obs, threshold=T, smooth=(5, 0.1, 0), **kw) == receptor_edges(f, obs, threshold=T, **kw), what
                # and the planes are the log-catches of the definition
                want_p = S.planes_and_values(f, obs.matrix, obs.weber, obs.floor, E.ACHROMATIC[obs.name], ch, sigma, D, (1, 1.0, 0), key=(H, W))[0]
                err = S.plane_error(planes, want_p, obs.n_receptors, obs.weber, E.ACHROMATIC[obs.name][1], ch)
                assert planes.shape == want_p.shape and err.max() <= S.BOUND, (what, float(err.max()))


# ------------------------------------------------------------------------------------------------ exact properties
def test_a_flat_frame_keeps_its_planes_and_gives_a_zero_record_and_a_black_map():
    H, W = 33, 70
    flat = np.stack([np.broadcast_to(np.array(c, np.uint8), (H, W, 3)) for c in ((200, 60, 60), (0, 0, 0), (255, 255, 255), (12, 9, 40))])
    for k, obs in enumerate(_observers()):
        for j, ch in enumerate(E.CHANNELS):
            kw = _kw(obs, ch, (0.0, 1.0)[(k + j) % 2], (1, 8)[j % 2])
            before = _all(flat, obs, kw, (1, 0.5, 0))[3]
            for smooth in S.SETTINGS + ((4, 0.7, 8),):
                plain, recs, v, planes = _all(flat, obs, kw, smooth, "plain", 255.0, 0.0)
                assert planes.tobytes() == before.tobytes() and not v.any() and not plain.any(), (obs.name, ch, smooth)
                assert all(_zero_record(r, H * W) for r in recs), (obs.name, ch, smooth)


@pytest.mark.parametrize("vertical,c", [(True, 64), (True, 50), (False, 32), (False, 21)])
def test_a_straight_seam_is_a_fixed_point_at_keep_up_to_a_half(vertical, c):
    """Two flat colours with the seam on a tile seam of the 64 x 32 tiling (column 64, row 32) and off it: at KEEP <= 0.5 every
    window holds at least m pixels of the pixel's own colour, t = 0, and neither the planes nor the edge values move."""
    from animal_vision_amd.metrics import receptor_edges_values

    H, W = 70, 130
    f = np.empty((H, W, 3), np.uint8)
    if vertical:
        f[:, :c], f[:, c:] = (200, 60, 60), (60, 200, 60)
    else:
        f[:c], f[c:] = (200, 60, 60), (60, 200, 60)
    combos = [(R, keep, it) for R in range(1, 6) for keep in (0.5, 0.25) for it in (1, 3)]
    obs3 = _observers()
    for n, smooth in enumerate(combos):
        obs, ch = obs3[n % 3], E.CHANNELS[(n // 3) % 3]  # every observer and channel meets every R
        kw = _kw(obs, ch, 0.0, 1)
        before = _all(f, obs, kw, (1, 0.5, 0))
        assert before[2].any() and before[2].tobytes() == receptor_edges_values(f, obs, **kw).tobytes()
        got = _all(f, obs, kw, smooth)
        what = (obs.name, ch, smooth, vertical, c)
        assert got[3].tobytes() == before[3].tobytes() and got[2].tobytes() == before[2].tobytes(), what
        assert got[0].tobytes() == before[0].tobytes() and got[1] == before[1], what


@pytest.mark.parametrize("H,W", [(5, 7), (70, 130)])
def test_greys_stay_chromatically_zero_with_and_without_blur(H, W):
    g = np.stack(A.grey_frames(H, W))
    for k, obs in enumerate(_observers()):
        for sigma, D, smooth in ((0.0, 1, S.SETTINGS[k]), (1.0, 2, S.SETTINGS[(k + 3) % 5]), (4.0, 1, (5, 0.33, 3))):
            plain, recs, v, planes = _all(g, obs, _kw(obs, "chromatic", sigma, D), smooth, "plain", 255.0, 0.0)
            assert not v.any() and not plain.any() and all(_zero_record(r, H * W) for r in recs), (obs.name, sigma, D, smooth, float(v.max()))
            assert all(planes[:, 0].tobytes() == planes[:, i].tobytes() for i in range(1, obs.n_receptors)), (obs.name, sigma, smooth)
            both = _all(g, obs, _kw(obs, "either", sigma, D), smooth)[3]
            assert all(both[:, 0].tobytes() == both[:, i].tobytes() for i in range(1, obs.n_receptors)), (obs.name, sigma, smooth)
            assert (H, W) == (5, 7) or _all(g, obs, _kw(obs, "achromatic", sigma, D), smooth)[2].any()


# ------------------------------------------------------------------------------------------------ batches, groups and alignment
def test_a_frame_is_bit_equal_alone_in_a_batch_and_from_an_offset_buffer():
    H, W = 33, 70
    f = E.frames(H, W)
    k = 3
    for obs, (sigma, D), ch, smooth in zip(_observers(), ((1.0, 8), (0.0, 1), (0.0, 2)), ("either", "chromatic", "achromatic"), ((5, 0.33, 3), (1, 0.5, 2), (3, 0.3, 1))):
        kw = _kw(obs, ch, sigma, D)
        alone = _all(f[k], obs, kw, smooth)
        assert alone[2].any()

        def same(got, j, what):
            assert got[0][j].tobytes() == alone[0].tobytes() and got[1][j] == alone[1], what
            assert got[2][j].tobytes() == alone[2].tobytes() and got[3][j].tobytes() == alone[3].tobytes(), what

        for place in range(3):  # as frame 0, 1 and 2 of a batch of three
            order = [(k + 1 + j) % 6 for j in range(2)]
            order.insert(place, k)
            same(_all(f[order], obs, kw, smooth), place, (obs.name, place))
        order = [(j * 5 + 1) % 6 for j in range(16)]  # a batch of 16
        got = _all(f[order], obs, kw, smooth)
        assert sum(o == k for o in order) >= 2
        for j in (i for i, o in enumerate(order) if o == k):
            same(got, j, (obs.name, j))
        for offsets in ((1, 1), (1, 0), (0, 1)):  # from buffers offset by one byte
            got = _all(f[k], obs, kw, smooth, offsets=offsets)
            assert got[0].tobytes() == alone[0].tobytes() and got[1] == alone[1] and got[2].tobytes() == alone[2].tobytes(), (obs.name, offsets)
            assert got[3].tobytes() == alone[3].tobytes(), (obs.name, offsets)


def test_a_batch_that_spans_two_scratch_groups():
    """The four-class observer, either: P = 5, 40 bytes of scratch a pixel.  At 1296 x 1296 the 1 GiB hold 15 frames (2^30 // (40 x
    1296^2) = 15, the partials taken off), so a batch of 16 is walked as 15 + 1: frame 3 lies in the first group, frame 15 alone in the
    second, and both equal the frame run on its own."""
    H = W = 1296
    assert (2 ** 30 - 16 * 8 * 21 * 44) // (40 * H * W) == 15  # 21 x 44 blocks of 62 x 30 a frame
    small = E.frames(33, 70)
    tile = lambda a: np.tile(a, (40, 19, 1))[:H, :W]  # noqa: E731
    x, other = tile(small[0]), tile(small[4])
    batch = np.empty((16, H, W, 3), np.uint8)
    batch[:] = other
    batch[3] = batch[15] = x
    obs = _observers()[2]
    kw = _kw(obs, "either", 0.0, 1)
    alone = _all(x, obs, kw, (1, 0.5, 1))
    got = _all(batch, obs, kw, (1, 0.5, 1), planes_of=(3, 15, 14))
    assert alone[2].any()
    for j, pj in ((3, 0), (15, 1)):
        assert got[0][j].tobytes() == alone[0].tobytes() and got[1][j] == alone[1] and got[2][j].tobytes() == alone[2].tobytes(), j
        assert got[3][pj].tobytes() == alone[3].tobytes(), j
    assert got[2][14].tobytes() == got[2][0].tobytes() != alone[2].tobytes() and got[1][14] == got[1][0]


# ------------------------------------------------------------------------------------------------ the record and the map: no tolerance
@pytest.mark.parametrize("H,W", [(5, 7), (33, 70), (70, 130)])
def test_record_and_map_follow_the_devices_own_values(H, W):
    from test_edges_gpu import _check_record

    f = E.frames(H, W)
    for k, obs in enumerate(_observers()):
        smooth, sigma, D = S.CASES[(H, W)][k]
        ch = E.CHANNELS[(k + 2) % 3]
        kw = _kw(obs, ch, sigma, D)
        for mode, G, T in (("heat", None, 1.0), ("plain", 2.5, 0.0), ("heat", 0.37, 2.3)):
            got, recs, v, _ = _all(f, obs, kw, smooth, mode, G, T)
            for i, name in enumerate(E.KINDS):
                what = (obs.name, ch, name, mode, G, T, H, W, smooth, sigma, D)
                assert np.array_equal(got[i], DE.de_map(v[i], f[i], 10.0 if G is None else G, T, mode)), what  # the dim grey is the unfiltered frame's
                _check_record(recs[i], v[i], T, D, what)


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("H,W,case", [(H, W, i) for (H, W), cases in S.CASES.items() for i in range(len(cases))])
def test_values_and_planes_against_the_float64_definition(H, W, case):
    from animal_vision_amd.metrics import receptor_edges_values, receptor_smooth_planes

    smooth, sigma, D = S.CASES[(H, W)][case]
    f = E.frames(H, W)
    worst_v, worst_p = (-1.0, ()), (-1.0, ())
    for obs in _observers():
        lw = E.ACHROMATIC[obs.name][1]
        for ch in E.CHANNELS:
            want_p, want_v, _ = S.planes_and_values(f, obs.matrix, obs.weber, obs.floor, E.ACHROMATIC[obs.name], ch, sigma, D, smooth, key=(H, W))
            _, _, v, planes = _all(f, obs, _kw(obs, ch, sigma, D), smooth)
            assert v.dtype == planes.dtype == np.float32 and v.shape == want_v.shape and planes.shape == want_p.shape
            assert np.isfinite(v).all() and (v >= 0).all() and np.isfinite(planes).all()
            dv = np.abs(v.astype(np.float64) - want_v).reshape(len(E.KINDS), -1).max(axis=1)
            dp = S.plane_error(planes, want_p, obs.n_receptors, obs.weber, lw, ch).reshape(len(E.KINDS), -1).max(axis=1)
            print(f"smooth {H}x{W} {smooth} sigma {sigma} step {D} {obs.name} {ch}: largest |device - yardstick| values {dv.max():.3e} ("
                  + ", ".join(f"{k} {d:.2e}" for k, d in zip(E.KINDS, dv)) + f"), planes {dp.max():.3e} ("
                  + ", ".join(f"{k} {d:.2e}" for k, d in zip(E.KINDS, dp)) + f"), largest value {want_v.max():.4f}")
            for i, name in enumerate(E.KINDS):
                worst_v = max(worst_v, (float(dv[i]), (obs.name, ch, name)))
                worst_p = max(worst_p, (float(dp[i]), (obs.name, ch, name)))
                assert dv[i] <= S.BOUND and dp[i] <= S.BOUND, (obs.name, ch, name, H, W, smooth, sigma, D, float(dv[i]), float(dp[i]))
            # the array entries give the same planes and values
            if ch == "either":
                kw = _kw(obs, ch, sigma, D)
                assert receptor_edges_values(f, obs, smooth=smooth, **kw).tobytes() == v.tobytes()
                kw.pop("step")
                assert receptor_smooth_planes(f, obs, smooth=smooth, **kw).tobytes() == planes.tobytes()
                assert receptor_smooth_planes(f[1], obs, smooth=smooth, **kw).tobytes() == planes[1].tobytes()
    print(f"smooth {H}x{W} {smooth} sigma {sigma} step {D}: the largest deviation: values {worst_v[0]:.3e} at {worst_v[1]}, planes {worst_p[0]:.3e} at "
          f"{worst_p[1]}; the bound {S.BOUND:g}")


def test_the_smoothing_takes_the_noise_and_keeps_the_seam():
    """The worked example of README: a two-tone frame with +-6 codes of noise, Dog, either, at 5:0.5:5."""
    from animal_vision_amd.metrics import observer_for, receptor_edges_values

    H, W, c = 64, 96, 48
    clean = np.empty((H, W, 3), np.uint8)
    clean[:, :c], clean[:, c:] = (120, 110, 90), (132, 121, 99)
    rng = np.random.default_rng(7)
    noisy = (clean.astype(np.int16) + rng.integers(-6, 7, clean.shape)).astype(np.uint8)
    dog = observer_for("Dog", (0.05, 0.05))
    kw = dict(achromatic=((1,), 0.1))
    off = np.ones((H, W), bool)
    off[:, c - 6 : c + 6] = False
    raw, smooth = receptor_edges_values(noisy, dog, **kw), receptor_edges_values(noisy, dog, smooth=(5, 0.5, 5), **kw)
    seam_clean = float(receptor_edges_values(clean, dog, **kw)[:, c - 1 : c + 1].mean())
    seam = float(smooth[:, c - 1 : c + 1].mean())
    print(f"noisy two-tone frame, Dog either: off-seam mean {raw[off].mean():.3f} -> {smooth[off].mean():.3f} JND at 5:0.5:5; the seam {seam:.3f}, "
          f"the clean frame's {seam_clean:.3f}")
    assert smooth[off].mean() < 0.5 * raw[off].mean() and seam > 2 * smooth[off].mean()


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing():
    import ctypes

    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, check_achromatic, check_smooth, observer_for
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 16, 16
    fb = H * W * 3
    d_in = ctx.upload(np.zeros(fb, np.uint8))
    d_out = ctx.upload(np.full(2 * fb, 0xAB, np.uint8))
    d_rec = ctx.upload(np.full(DELTA_E_RECORD_BYTES + 8, 0xAB, np.uint8))
    d_pl = ctx.upload(np.full(3 * H * W * 4 + 8, 0xAB, np.uint8))
    a, o, r, pl = d_in.ptr, d_out.ptr, d_rec.ptr, d_pl.ptr
    fn = _lib.lib.avx_receptor_edges_smooth_u8
    dog = observer_for("Dog", (0.05, 0.05))
    good, L = ctypes.byref(dog.desc()), ctypes.byref(check_achromatic(dog, ((1,), 0.1)))
    nan, inf = float("nan"), float("inf")

    def sm(**kw):
        d = check_smooth((3, 0.5, 2))
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)

    def call(hwc=a, n=1, h=H, w=W, obs=good, lm=L, channel=2, sigma=1.0, step=1, smooth=sm(), mode=0, gain=10.0, threshold=1.0, out=o, rec=r, val=None, planes=pl):
        return (hwc, n, h, w, obs, lm, channel, sigma, step, smooth, mode, gain, threshold, out, rec, val, planes)

    try:
        calls = [(call(smooth=s), words) for s, words in ((None, "smooth is NULL"), (sm(struct_size=20), "struct_size"), (sm(radius=0), "smoothing radius must be 1..5"),
                                                          (sm(radius=6), "smoothing radius"), (sm(keep=0.0), "smoothing keep must be above 0 and at most 1"),
                                                          (sm(keep=1.0000001), "smoothing keep"), (sm(keep=nan), "smoothing keep"), (sm(keep=inf), "smoothing keep"),
                                                          (sm(keep=-0.5), "smoothing keep"), (sm(iterations=-1), "smoothing iterations must be 0..8"),
                                                          (sm(iterations=9), "smoothing iterations"))]
        calls += [(c, "") for c in (call(sigma=0.19), call(sigma=nan), call(step=0), call(step=9), call(channel=3), call(lm=None, channel=1), call(obs=None),
                                    call(hwc=None), call(rec=None), call(n=0), call(n=17), call(h=0), call(mode=2), call(gain=0.0), call(threshold=-1.0),
                                    call(rec=r + 4), call(val=o + 2), call(out=a), call(planes=pl + 2), call(planes=a))]
        for args, words in calls:
            assert fn(ctx._h, *args, ctx.stream) == _lib.AVX_ERR_INVALID, args
            msg = _lib.lib.avx_last_error(ctx._h).decode()
            assert msg.startswith("avx_receptor_edges_smooth_u8:") and words in msg, (args, msg)
        ctx.sync()
        assert (ctx.download(d_out, (2 * fb,), np.uint8) == 0xAB).all() and (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8) == 0xAB).all()
        assert (ctx.download(d_pl, (3 * H * W * 4 + 8,), np.uint8) == 0xAB).all()
        # the ends are good calls: black is flat
        for args in (call(smooth=sm(radius=1, keep=1e-300, iterations=0), mode=1, gain=2.0), call(smooth=sm(radius=5, keep=1.0, iterations=8), mode=1, gain=2.0),
                     call(lm=None, channel=0, sigma=0.0, planes=None, mode=1, gain=2.0)):
            assert fn(ctx._h, *args, ctx.stream) == 0, args
            ctx.sync()
            assert not ctx.download(d_out, (fb,), np.uint8).any() and (ctx.download(d_out, (2 * fb,), np.uint8)[fb:] == 0xAB).all()
            assert (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8)[DELTA_E_RECORD_BYTES:] == 0xAB).all()  # nothing behind the record
            assert (ctx.download(d_pl, (3 * H * W * 4 + 8,), np.uint8)[3 * H * W * 4 :] == 0xAB).all()  # nor behind the three planes
    finally:
        for d in (d_in, d_out, d_rec, d_pl):
            d.free()


# ------------------------------------------------------------------------------------------------ the command
def _y4m_frames(path):
    """(W, H) and the payloads of a .y4m file, read by hand."""
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


def test_command_end_to_end(capsys, tmp_path):
    import _yuv_ref
    from animal_vision_amd import edges
    from animal_vision_amd.deltae import CSV_HEADER, format_row
    from animal_vision_amd.metrics import observer_for, receptor_edges_map
    from animal_vision_amd.renderers import VideoRenderer

    src = "synthetic:96x48:7"
    vr = VideoRenderer(read_path=src, write_path=None)
    vr.open()
    f = np.stack([vr.get_image() for _ in range(7)])
    vr.close()
    dog = observer_for("Dog", (0.05, 0.05))
    csv, y4m = tmp_path / "f.csv", tmp_path / "o.y4m"
    argv = [src, y4m, "--observer", "Dog", "--weber", "0.05,0.05", "--achromatic", "1:0.1", "--acuity", "1.0", "--smooth", "3:0.5:2", "--csv", csv, "--batch", "3",
            "--depth", "2"]
    assert edges.main([str(v) for v in argv]) == 0
    cap = capsys.readouterr()
    want, recs = receptor_edges_map(f, dog, achromatic=((1,), 0.1), acuity=1.0, smooth=(3, 0.5, 2))
    plain = receptor_edges_map(f, dog, achromatic=((1,), 0.1), acuity=1.0)[0]
    assert not np.array_equal(want, plain)  # the option does something
    assert cap.out == "" and "acuity 1 px, smooth 3:0.5x2, step 1)" in cap.err
    assert csv.read_text() == CSV_HEADER + "\n" + "".join(format_row(i, r) + "\n" for i, r in enumerate(recs))
    (W, H), frames = _y4m_frames(y4m)
    assert (W, H) == (96, 48) and len(frames) == 7
    payloads = _yuv_ref.encode(want)
    for i in range(7):
        assert np.array_equal(frames[i], payloads[i]), i
