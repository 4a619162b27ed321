"""The MST++ honeybee route (uint8 frame -> MST++ cube -> spectral integration -> honeybee tail) over every HoneyBee setting, and its
fused form (the catch planes formed in conv_out's epilogue, avx_honeybee_u8 source 2) at video sizes.

Every honeybee setting is checked against the oracle's tail fed with the network's own cube (pred.predict: the forward pass is
tests/test_mstpp.py's subject), to the honeybee tolerance: +-1 code, fewer than 5e-3 of the samples off.  The settings the source-2 tile
schedule does not take (falsecolor_uv_mixed, blurs wider than 3 taps) must go through the cube route (fp16, 32-wide channels-last cube
-> the plane schedule) instead of failing; the ones it takes must keep the fused route, whose planes and statistics are checked at
1080p and 4K, where the launch walks many tiles per workgroup."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAM = np.linspace(400.0, 700.0, 31, dtype=np.float32)
MAPPINGS = ("falsecolor", "custom_matrix", "opponent", "uv_purple_yellow", "falsecolor_uv_mixed")
ADAPTATIONS = ("white_patch", "gray_world", None)
SIGMAS = (0.0, 0.2, 0.5, 1.5)  # blur ksize 0, 3, 5, 11
CUSTOM = np.array([[0.9, 0.3, -0.1], [0.1, 0.8, 0.2], [0.4, -0.2, 0.7]], np.float32)


@pytest.fixture(scope="module")
def pred():
    from animal_vision_amd.ml import MSTPlusPlusPredictor

    return MSTPlusPlusPredictor(None, seed=0, half=True)


@pytest.fixture(scope="module")
def cubes(pred):
    """(H, W) -> (frame, the device's own cube of it as float32 (H, W, 31)): computed once per frame."""
    from animal_vision_amd.synthetic import structured_frame

    cache = {}

    def get(hw):
        if hw not in cache:
            frame = structured_frame(11 + hw[0], hw[0], hw[1])
            cache[hw] = (frame, pred.predict(frame))
        return cache[hw]

    return get


def _bee(pred, **kw):
    from animal_vision_amd.animals import HoneyBee

    return HoneyBee(hsi_model=pred, custom_matrix=CUSTOM, **kw)


def _want(oracle, cube, *, mapping, adaptation, sigma, reflectance=True):
    want, _ = oracle.honeybee_tail(*oracle.honeybee_catches(cube, LAM, reflectance=reflectance), np.uint8, adaptation=adaptation, mapping_mode=mapping,
                                   blur_sigma_px=sigma, custom_matrix=CUSTOM)
    return want


def _bee_close(got, want):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() < 5e-3, (int(d.max()), float((d > 0).mean()))


@pytest.mark.parametrize("hw", [(72, 88), (37, 45)])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("adaptation", ADAPTATIONS)
@pytest.mark.parametrize("mapping", MAPPINGS)
def test_every_setting_matches_the_oracle_tail_on_the_network_cube(pred, cubes, oracle, mapping, adaptation, sigma, hw):
    """HoneyBee(hsi_model=pred, ...).visualize over mapping x adaptation x blur; both frames are padded by the harness (-> 80 x 96, 48 x 48)."""
    frame, cube = cubes(hw)
    base, out = _bee(pred, mapping_mode=mapping, adaptation=adaptation, blur_sigma_px=sigma).visualize(frame)
    assert base is frame and out.shape == frame.shape and out.dtype == np.uint8
    _bee_close(out, _want(oracle, cube, mapping=mapping, adaptation=adaptation, sigma=sigma))


@pytest.mark.parametrize("mapping,sigma", [("opponent", 0.2), ("falsecolor_uv_mixed", 0.5)])
def test_radiance_cube_setting_matches_the_oracle_tail(pred, cubes, oracle, mapping, sigma):
    """assume_hsi_is_reflectance=False: the cube is taken as radiance (no illuminant folded into the weights)."""
    frame, cube = cubes((72, 88))
    _, out = _bee(pred, mapping_mode=mapping, blur_sigma_px=sigma, assume_hsi_is_reflectance=False).visualize(frame)
    _bee_close(out, _want(oracle, cube, mapping=mapping, adaptation="white_patch", sigma=sigma, reflectance=False))


@pytest.mark.parametrize("sigma", [0.0, 0.2])
@pytest.mark.parametrize("adaptation", ADAPTATIONS)
@pytest.mark.parametrize("mapping", MAPPINGS[:4])
def test_fused_route_equals_the_cube_route(pred, cubes, monkeypatch, mapping, adaptation, sigma):
    """Every setting the source-2 schedule takes: the catch planes of conv_out's epilogue are the cube route's bit for bit, so the frames are
    identical wherever the tail's statistics are order statistics (white patch: a maximum; none); gray world divides by a mean whose double
    partial sums are grouped differently: +-1 code."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    frame, _ = cubes((72, 88))
    op = _bee(pred, mapping_mode=mapping, adaptation=adaptation, blur_sigma_px=sigma)._operator()
    assert op.takes_catches()
    fused = pred.honeybee(frame, op)
    monkeypatch.setattr(_AVX, "_specfuse", False)
    plain = pred.honeybee(frame, op)
    if adaptation == "gray_world":
        d = np.abs(fused.astype(np.int16) - plain.astype(np.int16))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, (int(d.max()), float((d > 0).mean()))
    else:
        assert np.array_equal(fused, plain)


def test_route_selection(pred, cubes, monkeypatch):
    """The defaults (the benchmarked configuration) keep conv_out's spectral epilogue; the settings the source-2 schedule does not take do
    not call it (and return a frame instead of avx_honeybee_u8's source-2 error)."""
    from animal_vision_amd.animals import HoneyBee
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    calls = []
    real = _AVX.conv3x3_lds_spectral

    def counted(*a, **kw):
        calls.append(a[0].shape)
        return real(*a, **kw)

    monkeypatch.setattr(_AVX, "conv3x3_lds_spectral", counted)
    frame, _ = cubes((72, 88))
    assert HoneyBee()._operator().takes_catches()
    _, out = HoneyBee(hsi_model=pred).visualize(frame)
    assert len(calls) == 1 and out.shape == frame.shape
    for kw in ({"mapping_mode": "falsecolor_uv_mixed"}, {"blur_sigma_px": 0.5}):
        calls.clear()
        bee = HoneyBee(hsi_model=pred, **kw)
        assert not bee._operator().takes_catches()
        _, out = bee.visualize(frame)
        assert calls == [] and out.shape == frame.shape, kw


def test_a_new_operator_never_takes_a_dropped_ones_padded_clone(pred, cubes, oracle):
    """pred.honeybee caches each operator's 32-band clone: one operator after another (each dropped before the next is built, so a new one
    usually lands at the address of the last) must each be run with its own setting."""
    frame, cube = cubes((72, 88))
    for mapping in ("opponent", "falsecolor", "uv_purple_yellow", "custom_matrix", "opponent"):
        op = _bee(pred, mapping_mode=mapping)._operator()
        _bee_close(pred.honeybee(frame, op), _want(oracle, cube, mapping=mapping, adaptation="white_patch", sigma=0.2))
        del op


def _records(partials, n):
    """partials (records, 3, 2) float64-sized tensor of 16-byte {float min, max; double sum} records -> (min, max, sum), each (n, 3)."""
    raw = np.ascontiguousarray(partials.cpu().numpy()).view(np.uint8).reshape(partials.shape[0], 3, 16)[:n]
    mn = np.ascontiguousarray(raw[..., 0:4]).view(np.float32)[..., 0]
    mx = np.ascontiguousarray(raw[..., 4:8]).view(np.float32)[..., 0]
    sm = np.ascontiguousarray(raw[..., 8:16]).view(np.float64)[..., 0]
    return mn, mx, sm


@pytest.mark.parametrize("hw", [(1080, 1920), (2160, 3840)])
def test_epilogue_catch_planes_at_video_sizes(pred, hw):
    """conv_out's spectral epilogue at 1080p (padded to 1088 rows and cropped back) and 4K: many tiles per workgroup, statistics accumulated
    across tiles.  The planes are the staged integration of the cube the unfused route writes, bit for bit (the same float32 FMA chain), and
    within 1e-4 of a float64 integration of that cube; the records reduce to the planes' own min / max and to their float64 sum."""
    import torch

    from animal_vision_amd import uv
    from animal_vision_amd.animals import HoneyBee
    from animal_vision_amd.ml.predict import pad_amounts
    from animal_vision_amd.synthetic import structured_frame

    H, W = hw
    frame = structured_frame(5, H, W)
    op32 = HoneyBee()._operator().padded_clone(32)
    dev = torch.from_numpy(frame).to(pred.device)
    planes, partials, n = pred.model.forward_from_u8(dev, pad_amounts(H, W, pred.stride), spectral=op32.weights)
    got = planes.cpu().numpy()
    mn, mx, sm = _records(partials, n)
    del planes, partials
    assert got.shape == (3, H, W)
    assert 0 < n <= 8 * torch.cuda.get_device_properties(pred.device).multi_processor_count
    cube = pred.predict_device_nhwc(dev).cpu().numpy()
    del dev
    assert cube.shape == (H, W, 32) and cube.dtype == np.float16 and not cube[..., 31].any()
    staged, stats = uv.spectral_integrate(cube, op32.weights, return_stats=True)
    assert np.array_equal(got.view(np.uint32), staged.view(np.uint32)), int((got != staged).sum())
    del staged
    w64 = op32.weights.astype(np.float64).T
    want = np.empty((3, H, W), np.float64)
    for r in range(0, H, 270):
        want[:, r : r + 270] = (cube[r : r + 270].reshape(-1, 32).astype(np.float64) @ w64).T.reshape(3, -1, W)
    del cube
    for k in range(3):
        err = float(np.abs(got[k] - want[k]).max())
        print(f"{H}x{W} plane {k}: {n} records, max |fused - float64| {err:.3e} of max {float(np.abs(want[k]).max()):.3e}")
        assert err <= 1e-4 * float(np.abs(want[k]).max()), (k, err)
        assert float(np.abs(want[k]).max()) > 0
        assert mn[:, k].min() == got[k].min() and mx[:, k].max() == got[k].max(), k
        assert stats[k, 0] == got[k].min() and stats[k, 1] == got[k].max(), k
        s64 = float(got[k].astype(np.float64).sum())
        assert abs(float(sm[:, k].sum()) - s64) <= 1e-9 * abs(s64), (k, float(sm[:, k].sum()), s64)


def test_1080p_cube_route_frame_matches_the_oracle(pred, oracle):
    """A 1080p frame through the cube route (falsecolor_uv_mixed, gray world, 5-tap blur): the plane schedule fed the fp16 cube.  Beyond
    +-1 code only where the oracle itself moves under float32-level jitter of the cube (tests/_sensitivity.py)."""
    from _sensitivity import outlier_stats

    from animal_vision_amd.synthetic import structured_frame

    frame = structured_frame(7, 1080, 1920)
    kw = dict(mapping="falsecolor_uv_mixed", adaptation="gray_world", sigma=0.5)
    _, out = _bee(pred, mapping_mode=kw["mapping"], adaptation=kw["adaptation"], blur_sigma_px=kw["sigma"]).visualize(frame)
    cube = pred.predict(frame)
    want = _want(oracle, cube, **kw)
    st = outlier_stats(out, want, lambda seed: _want(oracle, oracle.relative_jitter(seed)(cube), **kw))
    print("1080p cube route vs oracle:", st)
    assert st["frac_ne"] < 5e-3, st
    assert st["max"] <= 1 or st["unexplained_px"] == 0, st


@pytest.mark.parametrize("setting", [{"mapping_mode": "falsecolor_uv_mixed", "blur_sigma_px": 1.0}, {"adaptation": "gray_world"}])
def test_stream_op_equals_the_one_frame_route(pred, setting):
    """MstHoneybeeStreamOp (one slot stream per frame in flight) for a cube-route and a fused-route setting: byte-identical to pred.honeybee."""
    from animal_vision_amd.ml import MstHoneybeeStreamOp
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.synthetic import structured_frame

    H, W = 96, 160
    frames = [structured_frame(40 + i, H, W) for i in range(5)]
    bee = _bee(pred, **setting)._operator()
    op = MstHoneybeeStreamOp(pred, bee, H, W, depth=3)
    got = {}
    pipe = FramePipeline(op, H, W, depth=3)
    pipe.run(((i, f) for i, f in enumerate(frames)), lambda i, o: got.__setitem__(i, o))
    pipe.close()
    assert sorted(got) == list(range(5))
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], pred.honeybee(f, bee)), i


def test_band_count_other_than_the_networks_is_refused(pred, cubes):
    """A HoneyBee on a 16-band grid would integrate bands 0-15 of the 31-band cube once padded to 32: refused, on both entry points."""
    from animal_vision_amd.ml import MstHoneybeeStreamOp

    frame, _ = cubes((72, 88))
    bee = _bee(pred, hsi_band_centers_nm=np.linspace(400.0, 700.0, 16, dtype=np.float32))
    with pytest.raises(ValueError):
        bee.visualize(frame)
    with pytest.raises(ValueError):
        MstHoneybeeStreamOp(pred, bee._operator(), 96, 160, depth=3)
