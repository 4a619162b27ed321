"""GPU: frames batched through the plane-program UV species (planevm.DeviceBackend(frames=N), UVSpecies.visualize_batch,
SpeciesStreamOp / FramePipeline(batch=N)) against the single-frame path.

The criterion is IDENTITY: a batch is the same kernels with the frame as a grid dimension, every statistic of the reference is
per frame, and a frame's reductions are formed with the single-frame launch geometry -- so every byte must equal what
`visualize(frame)` returns, which tests/test_uv_species_gpu.py and test_uv_video_sizes_gpu.py pin against the oracle.  No tolerance
is involved anywhere in this file except the one direct oracle comparison, which uses that file's own criterion."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPECIES = ["anableps", "anchovy", "damselfish", "dragonfly", "goldfish", "guppy", "heliconius", "hummingbird", "jumping_spider", "kestrel", "morpho",
           "pieris", "rat_uv", "reindeer"]


def _five(H, W, seed=0):
    """Five different frames; one all dark, one flat, one whose values are all <= 1: the per-frame statistics differ and the
    degenerate branch of safe_norm (range < 1e-9) occurs in some frames of a batch only."""
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    rng = np.random.default_rng(seed + H)
    return np.stack([structured_frame(seed + 1, H, W), np.zeros((H, W, 3), np.uint8), noise_frame(seed + 2, H, W), np.full((H, W, 3), 128, np.uint8),
                     rng.integers(0, 2, (H, W, 3), dtype=np.uint8)])


def _species(mod):
    from animal_vision_amd import animals

    return getattr(animals, animals.UV_CLASS[mod])()


def _singles(sp, frames, **kw):
    res = [sp.visualize(f, **kw) for f in frames]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def _same(got, want, what):
    for name, g, w in (("baseline", got[0], want[0]), ("out", got[1], want[1])):
        assert g.shape == w.shape and g.dtype == np.uint8, (what, name)
        if not np.array_equal(g, w):
            bad = [int(i) for i in range(len(w)) if not np.array_equal(g[i], w[i])]
            d = np.abs(g.astype(np.int16) - w.astype(np.int16))
            raise AssertionError(f"{what}: {name} differs from the single-frame path in frames {bad}: {int((d > 0).sum())} samples, max |d| = {int(d.max())}")


@pytest.mark.parametrize("mod", SPECIES + ["rat_uv_night"])
def test_batch_equals_single_frames(mod):
    """visualize_batch == N x visualize, byte for byte; a batch of one; a capacity-5 plan replayed with 3 frames; the same
    batch twice (the tickets of every frame's reductions are back at zero)."""
    kw = {"mode": "night"} if mod == "rat_uv_night" else {}
    sp = _species("rat_uv" if mod == "rat_uv_night" else mod)
    assert hasattr(sp, "visualize_batch")  # fails on a tree without the feature
    for H, W in ((96, 128), (270, 480)):
        frames = _five(H, W)
        want = _singles(sp, frames, **kw)
        _same(sp.visualize_batch(frames, **kw), want, (mod, H, W, "batch of 5"))
        _same(sp.visualize_batch(frames, **kw), want, (mod, H, W, "batch of 5, again"))
        _same(sp.visualize_batch(frames[2:3], **kw), (want[0][2:3], want[1][2:3]), (mod, H, W, "batch of 1"))
        _same(sp.visualize_batch(frames[1:4], capacity=5, **kw), (want[0][1:4], want[1][1:4]), (mod, H, W, "capacity 5, 3 frames"))
        _same(sp.visualize_batch(frames, capacity=2, **kw), want, (mod, H, W, "split into batches of 2"))


@pytest.mark.parametrize("mod,H,W,N", [("hummingbird", 1080, 1920, 4), ("reindeer", 1080, 1920, 4), ("kestrel", 1080, 1920, 4), ("anableps", 1080, 1920, 4),
                                       ("morpho", 1080, 1920, 4), ("hummingbird", 2160, 3840, 2)])
def test_batch_equals_single_frames_video_sizes(mod, H, W, N):
    """Several percentiles (hummingbird), Sobel (kestrel), remap (anableps), down_up (morpho) at the sizes video comes in; 8
    pixels per thread in the elementwise kernels."""
    sp = _species(mod)
    frames = _five(H, W, seed=7)[[0, 2, 1, 4][:N]]
    want = _singles(sp, frames)
    _same(sp.visualize_batch(frames), want, (mod, H, W, N))


def test_rat_uv_auto_mode_splits_the_batch_by_variant():
    from animal_vision_amd.animals import RatUV
    from animal_vision_amd.planevm import DeviceProbes

    sp = RatUV()
    H, W = 135, 240
    f = _five(H, W, seed=3)
    frames = np.stack([f[0], (f[0] // 6).astype(np.uint8), f[2], (f[2] // 8).astype(np.uint8), f[1], f[3]])
    variants = [sp.variant(x, DeviceProbes) for x in frames]
    assert "day" in variants and "night" in variants, variants  # both sides of the median threshold inside one batch
    want = _singles(sp, frames)
    _same(sp.visualize_batch(frames), want, "rat_uv auto")
    _same(sp.visualize_batch(frames, mode="auto"), want, "rat_uv auto (explicit)")


# ------------------------------------------------------------------ avx_ew_run_batch on its own ---------------------------------
def _factor(n):
    h = int(n ** 0.5)
    while n % h:
        h -= 1
    return h, n // h


# the builder of the recorded reduction program and the hit / miss counters live in tests/_ew_ref.py (test_ew_isa_gpu.py shares them)
from _ew_ref import reduction_program as _reduction_program  # noqa: E402
from _ew_ref import spec_stats as _spec_stats  # noqa: E402


@pytest.mark.parametrize("n", [(1 << 20) - 1, 1920 * 1080, 3840 * 2160 + 3])
def test_ew_run_batch_reductions_bit_equal(n, monkeypatch):
    """min, max, sum and mean over three frames of different content in one launch: each frame's four scalars, and its stored
    plane, are bit-equal to avx_ew_run on that frame -- through the generated kernel and through the interpreter, replayed
    twice (the tickets are left at zero).  The COL and ROW vectors are shared between the frames (stride 0)."""
    from animal_vision_amd import _lib
    from animal_vision_amd._lib import EW_PLANE, lib
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = _factor(n)
    F, NS = 3, 16
    rng = np.random.default_rng(n % 1000)
    x = np.stack([rng.standard_normal(n, dtype=np.float32), (rng.random(n, dtype=np.float32) * 1e3 - 7.0).astype(np.float32),
                  np.full(n, 0.25, np.float32)])
    col = np.linspace(0.5, 1.5, W, dtype=np.float32)
    row = np.linspace(-1.0, 1.0, H, dtype=np.float32)
    gains = np.array([1.0, -0.5, 3.0])
    d_x, d_y = ctx.upload(x), ctx.malloc(4 * n * F)
    d_col, d_row = ctx.upload(col), ctx.upload(row)
    d_sc = ctx.malloc(8 * NS * F)
    bufs = [d_x, d_y, d_col, d_row, d_sc]

    def fresh_scalars():
        sc = np.full((F, NS), np.nan)
        sc[:, 8] = gains
        ctx.upload(sc, d_sc)

    def planes(f):
        return [(d_x.ptr + 4 * n * f, 1, EW_PLANE["f32"]), (d_col.ptr, 1, EW_PLANE["col"]), (d_row.ptr, 1, EW_PLANE["row"]), (d_y.ptr + 4 * n * f, 1, EW_PLANE["f32"])]

    def read():
        ctx.sync()
        return ctx.download(d_sc, (F, NS), np.float64)[:, :4].copy(), ctx.download(d_y, (F, n), np.float32)

    try:
        results = {}
        for spec in (True, False):
            if spec:
                monkeypatch.delenv("AVX_EW_NO_SPEC", raising=False)
            else:
                monkeypatch.setenv("AVX_EW_NO_SPEC", "1")
            # reference: avx_ew_run frame by frame
            fresh_scalars()
            h0, m0 = _spec_stats()
            for f in range(F):
                p, keep = _reduction_program(H, W, planes(f), d_sc.ptr + 8 * NS * f, NS)
                ctx._check(lib.avx_ew_run(ctx._h, ctypes.byref(p), ctx.stream))
            want_sc, want_y = read()
            h1, m1 = _spec_stats()
            assert (h1 - h0, m1 - m0) == ((F, 0) if spec else (0, 0)), "the program's structure is recorded: it must hit its generated kernel"
            assert np.isfinite(want_sc).all() and len({tuple(r) for r in want_sc}) == F
            # NumPy's view of the same numbers, loosely: the reference itself is sane
            y0 = ((x[0].reshape(H, W) * col[None, :] + row[:, None]) * np.float32(gains[0])).ravel()
            assert want_sc[0, 0] == float(y0.min()) and want_sc[0, 1] == float(y0.max())  # no fusing: the same IEEE operations
            # float32 partial sums of a few dozen terms per thread, folded in double: 1e-5 of the sum of magnitudes is generous
            assert abs(want_sc[0, 2] - y0.sum(dtype=np.float64)) <= 1e-5 * np.abs(y0).sum(dtype=np.float64)
            assert abs(want_sc[0, 3] - x[0].mean(dtype=np.float64)) <= 1e-5 * np.abs(x[0]).mean(dtype=np.float64)
            # the batch: one launch, twice
            p, keep = _reduction_program(H, W, planes(0), d_sc.ptr, NS)
            fs = (ctypes.c_size_t * 4)(4 * n, 0, 0, 4 * n)
            for rep in range(2):
                fresh_scalars()
                ctx.memset(d_y, 0)
                ctx._check(lib.avx_ew_run_batch(ctx._h, ctypes.byref(p), F, fs, NS, ctx.stream))
                got_sc, got_y = read()
                assert np.array_equal(got_sc.view(np.uint64), want_sc.view(np.uint64)), (n, spec, rep, got_sc, want_sc)
                assert np.array_equal(got_y.view(np.uint32), want_y.view(np.uint32)), (n, spec, rep)
            results[spec] = want_sc
        assert np.array_equal(results[True].view(np.uint64), results[False].view(np.uint64))  # generated kernel == interpreter
        # refusals: too many frames, frames storing to one shared plane, reductions without a scalar table per frame
        for args in ((_lib.AVX_EW_MAX_FRAMES + 1, fs, NS), (0, fs, NS), (F, (ctypes.c_size_t * 4)(4 * n, 0, 0, 0), NS), (F, fs, 0), (F, None, NS)):
            assert lib.avx_ew_run_batch(ctx._h, ctypes.byref(p), args[0], args[1], args[2], ctx.stream) == _lib.AVX_ERR_INVALID, args[0]
        assert lib.avx_last_error(ctx._h)
    finally:
        for b in bufs:
            b.free()


def test_batched_plans_hit_the_generated_kernels():
    for mod in ("hummingbird", "reindeer"):
        sp = _species(mod)
        frames = _five(270, 480, seed=11)
        h0, m0 = _spec_stats()
        sp.visualize_batch(frames)
        h1, m1 = _spec_stats()
        assert h1 > h0 and m1 == m0, (mod, "a batched program missed its generated kernel", m1 - m0)


def test_batch_vs_oracle_reindeer():
    """The one direct tie to the oracle: the batched frames against oracle/np_backend.py per frame, with the criterion
    tests/test_uv_species_gpu.py uses for this species, on the kinds of frame that file uses (a structured frame, a noise frame
    and its smooth + noise mix).  The flat and all-dark frames of the identity tests are left out here on purpose: their band planes
    are constant up to rounding, safe_norm divides rounding noise by rounding noise, and the oracle's own output moves by tens of
    codes under float32-level jitter (tests/_sensitivity.py reports every differing pixel as unstable) -- a comparison with the
    oracle says nothing there, while identity with the single-frame path, asserted above on exactly those frames, does."""
    from _sensitivity import check_codes
    from oracle import np_backend

    sp = _species("reindeer")
    H, W = 270, 480
    rng = np.random.default_rng(H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = (127 + 100 * np.sin(xx / 9.0)[..., None] * np.cos(yy[..., None] / 7.0 + np.arange(3))).clip(0, 255)
    mix = (0.75 * smooth + 0.25 * rng.integers(0, 256, (H, W, 3))).astype(np.uint8)
    frames = np.stack([_five(H, W, seed=5)[0], _five(H, W, seed=5)[2], mix])
    bases, outs = sp.visualize_batch(frames)
    for i, frame in enumerate(frames):
        wbase, wout = np_backend.run(sp, frame)
        assert np.array_equal(bases[i], wbase), i
        check_codes(outs[i], wout, ("reindeer", "batch", i), lambda seed, frame=frame: np_backend.run_jittered(sp, frame, seed)[1])


# ------------------------------------------------------------------ pipeline ----------------------------------------------------
def _stream(op_factory, frames, H, W, batch, **kw):
    from animal_vision_amd.pipeline import FramePipeline

    op, close = op_factory(batch)
    pipe = FramePipeline(op, H, W, depth=3, batch=batch, **kw)
    got = []
    try:
        stats = pipe.run(iter(enumerate(frames)), lambda i, out: got.append((i, out)))
    finally:
        pipe.close()
        if close:
            close()
    assert stats.frames == len(frames)
    return got


@pytest.mark.parametrize("kw", [{}, {"split_compare": True, "split_baseline": True}, {"io_format": "i420"},
                                {"io_format": "i420", "split_compare": True, "split_baseline": True, "labels": None}])
def test_pipeline_batch4_equals_batch1(kw):
    """10 frames = two full batches and a partial one: exactly the frames the batch=1 pipeline emits, in the same order."""
    from animal_vision_amd.animals import Hummingbird
    from animal_vision_amd.animals._uv_species import SpeciesStreamOp
    from animal_vision_amd.synthetic import noise_frame, structured_frame
    from animal_vision_amd.yuv import rgb_to_i420

    H, W = 136, 240
    rgb = [structured_frame(k, H, W) if k % 3 else noise_frame(k, H, W) for k in range(10)]
    rgb[4] = np.zeros((H, W, 3), np.uint8)
    frames = [rgb_to_i420(f) for f in rgb] if kw.get("io_format") == "i420" else rgb
    sp = Hummingbird()

    def factory(batch):
        op = SpeciesStreamOp(sp, H, W, depth=3, batch=batch)
        return op, op.close

    want = _stream(factory, frames, H, W, 1, **kw)
    got = _stream(factory, frames, H, W, 4, **kw)
    assert [i for i, _ in got] == [i for i, _ in want] == list(range(10))
    for (i, g), (_, w) in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (kw, i)


def test_pipeline_batch4_dichromat():
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.synthetic import noise_frame

    H, W = 120, 200
    frames = [noise_frame(k, H, W) for k in range(10)]
    want = _stream(lambda b: (DichromatOp(Dog.SPEC), None), frames, H, W, 1, split_compare=True)
    got = _stream(lambda b: (DichromatOp(Dog.SPEC), None), frames, H, W, 4, split_compare=True)
    assert [i for i, _ in got] == list(range(10))
    for (i, g), (_, w) in zip(got, want):
        assert np.array_equal(g, w), i


# ------------------------------------------------------------------ refusals ----------------------------------------------------
def test_refusals(tmp_path):
    from animal_vision_amd import video
    from animal_vision_amd.animals import MantisShrimp, Reindeer
    from animal_vision_amd.animals._uv_species import SpeciesStreamOp
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.planevm import DeviceBackend

    with pytest.raises(ValueError):
        DeviceBackend(32, 32, frames=17)
    with pytest.raises(ValueError):
        DeviceBackend(32, 32, frames=0)
    with pytest.raises(NotImplementedError):
        DeviceBackend(32, 32, float_frames=True, frames=2)
    sp = Reindeer()
    with pytest.raises(NotImplementedError):
        sp.visualize_batch(np.zeros((2, 32, 32, 3), np.float32))
    with pytest.raises(NotImplementedError):
        sp.visualize_batch(np.zeros((2, 32, 32, 3), np.uint16))
    be = DeviceBackend(32, 32, frames=2)
    try:
        with pytest.raises(ValueError):
            be.run_device(n_frames=3)
        with pytest.raises(NotImplementedError):
            be.streak([be.load(r) for r in be.new_planes(3)], (0.5, 1.0, 2.0, 1.0))
    finally:
        be.close()
    # an op that cannot take the batch is refused when the pipeline is built, not at the first frame
    op = SpeciesStreamOp(sp, 32, 48, depth=2, batch=2)
    try:
        with pytest.raises(ValueError):
            FramePipeline(op, 32, 48, depth=2, batch=4)
    finally:
        op.close()
    # the species of the per-frame loop have no batched form
    with pytest.raises(ValueError):
        video.stream_op(MantisShrimp(), 32, 48, 3, batch=2)
    with pytest.raises(SystemExit) as e:
        video.main(["synthetic:48x32:3", str(tmp_path / "out.npy"), "--species", "Mantis Shrimp", "--batch", "2"])
    assert "--batch" in str(e.value)


def test_video_command_batch(tmp_path):
    """`video --batch 4` writes the frames `video` writes (7 frames: one full batch and a partial one)."""
    from animal_vision_amd import video

    for species in ("HummingBird", "Dog", "HoneyBee"):
        a, b = tmp_path / f"{species}_1.npy", tmp_path / f"{species}_4.npy"
        assert video.main(["synthetic:96x64:7", str(a), "--species", species, "--split-compare"]) == 0
        assert video.main(["synthetic:96x64:7", str(b), "--species", species, "--split-compare", "--batch", "4"]) == 0
        x, y = np.load(a), np.load(b)
        assert x.shape[0] == 7 and x.shape == y.shape and np.array_equal(x, y), species
