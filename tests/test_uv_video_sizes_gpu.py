"""GPU: the 14 plane-program UV species, MantisShrimp and HoneyBee against the oracle at video sizes (1080p, an odd 1079 x 1917, 4K).

Their kernels change code path with the frame size: plane programs take 8 pixels per thread from n >= 2^20 and sweep a capped grid several
times (csrc/ew.hip), the radix-select candidate pass sweeps dense tiles twice (csrc/select.hip), and the blur / resize / remap / Sobel tiles run
with many tiles per row and ragged right and bottom edges.  The other tests compare one device route with another at these sizes; here the
device is compared with the oracle itself.

Contract: the baseline is bit-exact for uint8 frames and within 2e-5 for float frames; the stylised uint8 frame is held
by tests/_sensitivity.check_codes, the stylised float frame by check_float (1e-4 before the encode).  Every check records its statistics as
test properties (pytest --junitxml)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPECIES = ["anableps", "anchovy", "damselfish", "dragonfly", "goldfish", "guppy", "heliconius", "hummingbird", "jumping_spider", "kestrel", "morpho",
           "pieris", "rat_uv", "reindeer"]
SIZES = [(1080, 1920), (1079, 1917)]
FRAMES = ["structured", "composite", "clipped"]
MANTIS_KW = {"default": {}, "noresample": dict(hsi_scale=1.0, panorama_scale=1.0), "scaled": dict(hsi_scale=0.5, panorama_scale=1.3)}
# The clipped frame's blown-out block puts these cases' categorical decisions on exact ties over most of the block: the jittered oracle moves
# 1.7-2.8 % of the frame's pixels by >= 2 codes, so check_codes' fraction caps (0.2 % beyond +-1) cannot hold even for a correct device.
# They run in test_clipped_frame_where_the_oracle_is_ill_conditioned instead (measured on an MI355X: every sample beyond +-1 inside the
# oracle's own unstable mask).
ILL_CONDITIONED = {("dragonfly", (1079, 1917), "clipped"), ("hummingbird", (1079, 1917), "clipped"), ("mantis noresample", (1080, 1920), "clipped"),
                   ("mantis noresample", (1079, 1917), "clipped")}


def _frame(kind: str, H: int, W: int) -> np.ndarray:
    """uint8 test frames: flat bars (ties, dense percentile tiles), the smooth + noise composite of the smaller tests, and a frame with
    clipped highlights and deep shadows (the clips and the tone-compression knees)."""
    from animal_vision_amd.synthetic import structured_frame

    if kind == "structured":
        return structured_frame(1, H, W)
    rng = np.random.default_rng(H * 3 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = (127 + 100 * np.sin(xx / 9.0)[..., None] * np.cos(yy[..., None] / 7.0 + np.arange(3))).clip(0, 255)
    if kind == "composite":
        return (0.75 * smooth + 0.25 * rng.integers(0, 256, (H, W, 3))).astype(np.uint8)
    assert kind == "clipped"
    f = 1.3 * smooth + 0.2 * rng.integers(0, 256, (H, W, 3)) - 45.0  # ~8 % of the samples clip at 255, a few % at 0
    f[: H // 6, : W // 5] = 255  # blown-out sky
    # crushed shadows at codes 1-3, not an all-black block: hummingbird's x / (x + y + z + 1e-8) and dragonfly are ill-conditioned on exact
    # black (at 1079 x 1917 the jittered oracle moved 58,333 / 50,451 pixels of such a block by >= 2 codes, far over check_codes' caps)
    f[H - H // 6 :, W - W // 5 :] = rng.integers(1, 4, (H // 6, W // 5, 3))
    return f.clip(0, 255).astype(np.uint8)


def _species(mod):
    from animal_vision_amd import animals

    return getattr(animals, animals.UV_CLASS[mod])()


def _record(record_property, key, st):
    record_property(key, {k: v for k, v in st.items() if k != "unexplained_at"})


def _codes(got, want, what, rerun, runs=6):
    from _sensitivity import check_codes

    st = check_codes(got, want, what, rerun, runs=runs)
    # every sample beyond +-1 sits in the dilated unstable mask (check_codes asserts it): at stable pixels |d| <= 1
    st["max_stable"] = st["max"] if st["outlier_px"] == 0 else min(st["max"], 1)
    return st


def _float_frames(u8: np.ndarray, H: int):
    """float32 in [0, 1] and in [0, 255] at every size, float64 in [0, 1] at 1080p."""
    out = [("f32_01", (u8 / 255.0).astype(np.float32)), ("f32_255", u8.astype(np.float32))]
    if H == 1080:
        out.append(("f64_01", u8 / 255.0))
    return out


# ---- the 14 plane-program species ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", SPECIES)
def test_species_uint8_video_sizes_vs_oracle(mod, record_property):
    from oracle import np_backend

    sp = _species(mod)
    shapes = SIZES + ([(2160, 3840)] if mod in ("hummingbird", "reindeer") else [])
    for H, W in shapes:
        for kind in FRAMES if H < 2160 else ["structured", "composite"]:
            if (mod, (H, W), kind) in ILL_CONDITIONED:
                continue
            frame = _frame(kind, H, W)
            base, out = sp.visualize(frame)
            wbase, want = np_backend.run(sp, frame)
            assert base.dtype == out.dtype == np.uint8 and out.shape == frame.shape
            assert np.array_equal(base, wbase), (mod, (H, W), kind, "baseline")
            st = _codes(out, want, (mod, (H, W), kind), lambda seed: np_backend.run_jittered(sp, frame, seed)[1])
            _record(record_property, f"u8 {H}x{W} {kind}", st)


@pytest.mark.parametrize("mod", SPECIES)
def test_species_float_video_sizes_vs_oracle(mod, record_property):
    from _sensitivity import check_float
    from oracle import np_backend

    sp = _species(mod)
    for (H, W), kind in zip(SIZES, ("structured", "composite")):
        for name, frame in _float_frames(_frame(kind, H, W), H):
            base, out = sp.visualize(frame)
            wbase, want = np_backend.run(sp, frame)
            assert base.dtype == out.dtype == wbase.dtype == want.dtype == frame.dtype and out.shape == frame.shape
            np.testing.assert_allclose(base, wbase, rtol=0, atol=2e-5, err_msg=f"{mod} {name} {H}x{W} baseline")
            st = check_float(out, want, (mod, (H, W), kind, name), lambda seed: np_backend.run_jittered(sp, frame, seed)[1])
            _record(record_property, f"{name} {H}x{W} {kind}", st)


def test_rat_uv_auto_takes_the_night_plan_at_1080p(record_property):
    from animal_vision_amd.animals import RatUV
    from oracle import np_backend

    sp = RatUV()
    dark = (_frame("composite", 1080, 1920) // 6).astype(np.uint8)
    assert sp.variant(dark, np_backend.NumpyProbes) == "night"
    base, out = sp.visualize(dark, mode="auto")
    wbase, want = np_backend.run(sp, dark)
    assert np.array_equal(base, wbase)
    _record(record_property, "auto->night", _codes(out, want, "auto->night", lambda seed: np_backend.run_jittered(sp, dark, seed)[1]))


# ---- MantisShrimp ----------------------------------------------------------------------------------------------------------------------
def _mantis_rerun(frame, kw):
    from oracle import cpu_ref

    return lambda seed: cpu_ref.mantis_visualize(frame, _jit=cpu_ref.relative_jitter(seed), **kw)[1]


@pytest.mark.parametrize("tag", list(MANTIS_KW))
def test_mantis_uint8_video_sizes_vs_oracle(tag, record_property):
    from animal_vision_amd.animals import MantisShrimp
    from oracle import cpu_ref

    kw = MANTIS_KW[tag]
    m = MantisShrimp(**kw)
    cases = [(s, k) for s in SIZES for k in FRAMES] + ([((2160, 3840), "structured")] if tag == "default" else [])
    for (H, W), kind in cases:
        if ("mantis " + tag, (H, W), kind) in ILL_CONDITIONED:
            continue
        frame = _frame(kind, H, W)
        base, out = m.visualize(frame)
        wbase, want = cpu_ref.mantis_visualize(frame, **kw)
        assert np.array_equal(base, wbase), (tag, (H, W), kind, "baseline")
        # 12 probe runs, not 6: mantis' argmax band ties to a few ulp at a handful of pixels per video frame, and six draws can miss one (default,
        # 1079 x 1917 composite, pixel (729, 641): the top two bands 3 ulp apart, moved by jitter seeds 6, 7, 12, 13, ... but by none of 0-5)
        _record(record_property, f"u8 {H}x{W} {kind}", _codes(out, want, (tag, (H, W), kind), _mantis_rerun(frame, kw), runs=12))


def test_mantis_float_video_sizes_vs_oracle(record_property):
    from _sensitivity import check_float
    from animal_vision_amd.animals import MantisShrimp
    from oracle import cpu_ref

    m = MantisShrimp()
    for (H, W), kind in zip(SIZES, ("structured", "composite")):
        for name, frame in _float_frames(_frame(kind, H, W), H):
            base, out = m.visualize(frame)
            wbase, want = cpu_ref.mantis_visualize(frame)
            assert base.dtype == out.dtype == want.dtype == frame.dtype and out.shape == frame.shape
            np.testing.assert_allclose(base, wbase, rtol=0, atol=2e-5, err_msg=f"mantis {name} {H}x{W} baseline")
            _record(record_property, f"{name} {H}x{W} {kind}", check_float(out, want, ("mantis", (H, W), name), _mantis_rerun(frame, {})))


def _subnormal_gradient_frame() -> np.ndarray:
    """Zeros with columns 0-11 at 1.0 (a non-zero P95) and a 4 x 4 patch of 1e-19 with one hole: the Sobel pair of the band mean is
    non-zero but gx^2 + gy^2 is below FLT_MIN at some pixels of the patch's rim."""
    f = np.zeros((64, 64, 3), np.float32)
    f[:, :12] = 1.0
    f[40:44, 40:44] = 1e-19
    f[41, 41] = 0.0
    return f


def _oracle_sobel_pair(frame, kw):
    """The Sobel pair of cpu_ref.mantis_visualize (same helper calls, hsi_scale = panorama_scale = 1)."""
    from oracle import cpu_ref as O

    assert kw["hsi_scale"] == 1.0 and kw["panorama_scale"] == 1.0
    lam = np.linspace(300.0, 700.0, 81, dtype=np.float32)
    hsi = O.classic_rgb_to_hsi_lobes(O.uv_srgb_to_linear(O.to_float01(frame)), lam)
    _, s_norm = O.mantis_barcode(O.mantis_band_stack(hsi, lam))
    broad = np.mean(s_norm, axis=2).astype(np.float32)
    return O.cv_sobel3(broad, 1, 0), O.cv_sobel3(broad, 0, 1)


@pytest.mark.parametrize("fuse", ["fused", "unfused"])
def test_mantis_subnormal_gradients_stay_finite(fuse, monkeypatch, record_property):
    """csrc/mantis.hip::pol_gain_of on a gradient whose squared norm is subnormal: 1 / r2 overflows unless the direction is taken from
    rescaled components.  The oracle's arctan2 route is finite there; the device must be too, and within the float contract."""
    from _sensitivity import check_float
    from animal_vision_amd.animals import MantisShrimp
    from oracle import cpu_ref

    kw = dict(hsi_scale=1.0, panorama_scale=1.0)
    frame = _subnormal_gradient_frame()
    gx, gy = _oracle_sobel_pair(frame, kw)
    r2 = gx * gx + gy * gy
    n_sub = int(((r2 > 0) & (r2 < np.finfo(np.float32).tiny)).sum())
    assert n_sub > 0, "the frame no longer produces subnormal squared gradients in the oracle"
    if fuse == "unfused":
        monkeypatch.setenv("AVX_MANTIS_FUSE", "0")
    base, out = MantisShrimp(**kw).visualize(frame)
    wbase, want = cpu_ref.mantis_visualize(frame, **kw)
    assert np.isfinite(want).all()
    np.testing.assert_allclose(base, wbase, rtol=0, atol=2e-5)
    st = check_float(out, want, ("mantis subnormal", fuse), _mantis_rerun(frame, kw))
    st["subnormal_r2_px"] = n_sub
    _record(record_property, fuse, st)


# ---- HoneyBee as coded (analytic lobes, opponent mapping) ----------------------------------------------------------------------------
def test_honeybee_float_video_sizes_vs_oracle(record_property):
    from _sensitivity import check_float
    from animal_vision_amd.animals import HoneyBee
    from oracle import cpu_ref

    def rerun(frame):
        lam = np.linspace(400.0, 700.0, 31, dtype=np.float32)
        catches = cpu_ref.honeybee_catches(cpu_ref.classic_rgb_to_hsi_lobes(cpu_ref.to_float01(frame), lam), lam)

        def run(seed):  # the jitter enters at the catches and travels through adaptation, blur, percentiles and the opponent mapping
            jit = cpu_ref.relative_jitter(seed)
            return cpu_ref.honeybee_tail(*[jit(c) for c in catches], frame.dtype)[0]

        return run

    bee = HoneyBee()
    for (H, W), kind in zip(SIZES, ("structured", "composite")):
        for name, frame in _float_frames(_frame(kind, H, W), H):
            base, out = bee.visualize(frame)
            _, want = cpu_ref.honeybee_visualize(frame)
            assert out.dtype == want.dtype == frame.dtype and out.shape == frame.shape
            np.testing.assert_allclose(base, frame, rtol=0, atol=2e-5)
            _record(record_property, f"{name} {H}x{W} {kind}", check_float(out, want, ("honeybee", (H, W), name), rerun(frame)))


# ---- plane-program reductions at scale (the interpreter) -----------------------------------------------------------------------------
# n = 2^20 - 1 and 2^20 straddle the 4 -> 8 pixels-per-thread switch; 1080p runs ~1,000 workgroups with a ragged last one, 4K sweeps the
# capped grid several times; 4K + 3 leaves a ragged last vector.
REDUCE_SHAPES = [(1023, 1025), (1024, 1024), (1080, 1920), (1079, 1917), (2160, 3840), (1, 2160 * 3840 + 3)]


@pytest.mark.parametrize("shape", REDUCE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plane_program_reductions_at_video_sizes(shape):
    """min / max / mean of one recorded program and a percentile over three planes taken together, vs NumPy, replayed twice.

    mean: ew.hip sums each workgroup's values in float32, folds the float32 partials in double and returns float32(sum) / n, like
    ndarray.mean() of a float32 array.  The values are positive, so the float32 partial sums are off by at most (chain length) * 2^-24 of the
    total; the longest chain (per-thread sweeps + 8-register merge + wave shuffle + block fold) is far below 64 additions at these sizes."""
    from animal_vision_amd.planevm import DeviceBackend

    H, W = shape
    n = H * W
    be = DeviceBackend(H, W)
    try:
        rng = np.random.default_rng(n)
        a = rng.random((H, W), dtype=np.float32)
        b = rng.random((H, W), dtype=np.float32) + np.float32(0.1)
        a[H // 2, W // 3] = np.float32(1.5)  # a unique max and min away from the first and last workgroup
        b[H - 1, W - 1] = np.float32(0.03125)
        pa, pb = be.new_planes(2)
        be.ctx.upload(a, pa.buf.view(pa.offset, a.nbytes))
        be.ctx.upload(b, pb.buf.view(pb.offset, b.nbytes))
        A, B = be.load(pa), be.load(pb)
        expr = A * B + 0.25
        mn, mx, mean = be.min(expr), be.max(expr), be.mean(expr)
        p = be.percentile([expr, A, B], 95.0)
        be.flush()
        slots = [v.imm for v in (mn, mx, mean, p)]

        def replay():
            for fn in be.plan:
                fn(be.ctx.stream)
            return be.ctx.download(be.scalars, (be.N_SCALARS,), np.float64)[slots]

        got1, got2 = replay(), replay()
    finally:
        be.close()
    e = a * b + np.float32(0.25)
    assert got1[0] == float(e.min()) and got1[1] == float(e.max()), (shape, got1[:2], e.min(), e.max())
    want_mean = float(np.float32(e.sum(dtype=np.float64)) / np.float32(n))
    assert abs(got1[2] - want_mean) <= 64 * 2.0 ** -24 * want_mean, (shape, got1[2], want_mean)
    want_p = np.percentile(np.stack([e, a, b]), 95.0)
    assert want_p.dtype == np.float32 and got1[3] == float(want_p), (shape, got1[3], float(want_p))
    assert np.array_equal(got1, got2), ("second replay differs: ticket / partials not left clean", shape, got1, got2)


class OverFractionCap(Exception):
    pass


@pytest.mark.xfail(strict=True, raises=OverFractionCap,
                   reason="the oracle is ill-conditioned on the clipped frame's flat block; measured device vs oracle: dragonfly 1079x1917 19,298 "
                          "pixels beyond +-1 (frac 3.1e-3) of 50,450 unstable, hummingbird 1079x1917 54,909 (2.3e-2) of 58,345, mantis noresample "
                          "1080p 28,641 (9.3e-3) of 35,714, mantis noresample 1079x1917 27,427 (8.9e-3) of 34,450; none outside the dilated unstable mask")
@pytest.mark.parametrize("case", sorted(ILL_CONDITIONED), ids=lambda c: f"{c[0].replace(' ', '_')}-{c[1][0]}x{c[1][1]}")
def test_clipped_frame_where_the_oracle_is_ill_conditioned(case, record_property):
    """Baseline bit-exact and every sample beyond +-1 where the oracle itself is unstable (hard assertions); check_codes' fraction caps
    are expected to fail (strict xfail: if they ever hold, this case belongs back in the main tests)."""
    from _sensitivity import check_codes, outlier_stats
    from animal_vision_amd.animals import MantisShrimp
    from oracle import cpu_ref, np_backend

    name, (H, W), kind = case
    frame = _frame(kind, H, W)
    if name.startswith("mantis "):
        kw = MANTIS_KW[name.split()[1]]
        base, out = MantisShrimp(**kw).visualize(frame)
        wbase, want = cpu_ref.mantis_visualize(frame, **kw)
        rerun = _mantis_rerun(frame, kw)
    else:
        sp = _species(name)
        base, out = sp.visualize(frame)
        wbase, want = np_backend.run(sp, frame)
        rerun = lambda seed: np_backend.run_jittered(sp, frame, seed)[1]  # noqa: E731
    assert np.array_equal(base, wbase), (case, "baseline")
    runs = {}

    def rerun_once(seed):  # check_codes repeats outlier_stats' probe: the jittered frames are computed once
        if seed not in runs:
            runs[seed] = rerun(seed)
        return runs[seed]

    st = outlier_stats(out, want, rerun_once)
    _record(record_property, f"u8 {H}x{W} {kind}", st)
    assert st.get("unexplained_px", 0) == 0 and st["outlier_px"] <= st.get("unstable_px", 0), (case, st)
    try:
        check_codes(out, want, case, rerun_once)
    except AssertionError as e:
        raise OverFractionCap(str(e)[:300]) from None
