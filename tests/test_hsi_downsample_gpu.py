"""HoneyBee on MST++ at reduced network resolution: HoneyBee(hsi_model=pred, hsi_downsample=True, hsi_scale=s) runs the
network on the frame reduced by s (uint8 INTER_AREA), enlarges the three catch planes (avx_catch_planes_up: cv2's float32 INTER_LINEAR and
the planes' statistics in one launch) and runs the honeybee tail at full size.

The kernel is held to the existing resize entry point bit for bit and to NumPy's statistics; the route to a composition of entry points
that existed before it (byte-identical where the tail's statistics are order statistics) and to the CPU oracle's chain (the honeybee
tolerance); the stream operator and the `video` command to HoneyBee.visualize byte for byte."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAM = np.linspace(400.0, 700.0, 31, dtype=np.float32)
CUSTOM = np.array([[0.9, 0.3, -0.1], [0.1, 0.8, 0.2], [0.4, -0.2, 0.7]], np.float32)
UP_SHAPES = [((1, 1), (5, 7)), ((2, 3), (5, 7)), ((7, 9), (72, 88)), ((36, 44), (72, 88)), ((24, 33), (97, 131)), ((6, 6), (64, 64)),
             ((64, 64), (64, 64))]
CASES = [((72, 88), 0.5), ((97, 131), 0.25), ((72, 88), 0.1)]  # reduced to 36 x 44, 24 x 33 and 7 x 9: padded to 48 x 48, 32 x 48 and 16 x 16
SETTINGS = [("opponent", "white_patch", 0.2), ("falsecolor", None, 0.0), ("custom_matrix", "gray_world", 0.2), ("falsecolor_uv_mixed", "white_patch", 0.5)]


@pytest.fixture(scope="module")
def pred():
    from animal_vision_amd.ml import MSTPlusPlusPredictor

    return MSTPlusPlusPredictor(None, seed=0, half=True)


def _frame(hw):
    from animal_vision_amd.synthetic import structured_frame

    return structured_frame(11 + hw[0], hw[0], hw[1])


def _bee(pred, mapping="opponent", adaptation="white_patch", sigma=0.2, scale=None):
    from animal_vision_amd.animals import HoneyBee

    kw = {} if scale is None else {"hsi_downsample": True, "hsi_scale": scale}
    return HoneyBee(hsi_model=pred, custom_matrix=CUSTOM, mapping_mode=mapping, adaptation=adaptation, blur_sigma_px=sigma, **kw)


def _bee_close(got, want):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print("max code difference", int(d.max()), "share", float((d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() < 5e-3, (int(d.max()), float((d > 0).mean()))


# ---------------------------------------------------------------- 1. the kernel against avx_resize_hwc and NumPy ----------------
def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _planes_up(small, H, W, offset=0):
    """avx_catch_planes_up of (3, h, w) float32 planes -> ((3, H, W) planes, (n, 3) min, max, sum); planes_out starts `offset` bytes into its buffer."""
    from animal_vision_amd._lib import lib
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    _, h, w = small.shape
    nbytes = 3 * H * W * 4
    d_in, d_out, d_part = ctx.upload(small), ctx.malloc(nbytes + 64), ctx.malloc(8 * _cus() * 3 * 16)
    n = ctypes.c_int(0)
    try:
        ctx.memset(d_out, 0xFF)
        ctx._check(lib.avx_catch_planes_up(ctx._h, d_in.ptr, h, w, d_out.ptr + offset, H, W, d_part.ptr, ctypes.byref(n), ctx.stream))
        planes = ctx.download(d_out.view(offset, nbytes), (3, H, W), np.float32)
        guard = ctx.download(d_out, (nbytes + 64,), np.uint8)
        assert (guard[:offset] == 0xFF).all() and (guard[offset + nbytes:] == 0xFF).all()  # nothing written outside the planes
        assert 1 <= n.value <= 8 * _cus()
        rec = ctx.download(d_part, (n.value, 3, 16), np.uint8)
    finally:
        for b in (d_in, d_out, d_part):
            b.free()
    mn = np.ascontiguousarray(rec[..., 0:4]).view(np.float32)[..., 0]
    mx = np.ascontiguousarray(rec[..., 4:8]).view(np.float32)[..., 0]
    sm = np.ascontiguousarray(rec[..., 8:16]).view(np.float64)[..., 0]
    return planes, mn, mx, sm


def _small_planes(h, w, seed):
    rng = np.random.default_rng(seed)
    small = rng.standard_normal((3, h, w)).astype(np.float32) * np.float32(3.0)  # negative values too
    small[1] = np.float32(-0.375)                                                # a constant plane
    return small


@pytest.mark.parametrize("hw,HW", UP_SHAPES)
def test_planes_equal_the_resize_entry_point_and_records_reduce_to_numpy(hw, HW):
    from animal_vision_amd import geometry

    (h, w), (H, W) = hw, HW
    small = _small_planes(h, w, seed=h * 131 + W)
    planes, mn, mx, sm = _planes_up(small, H, W)
    for k in range(3):
        want = geometry.resize(small[k], (W, H), geometry.INTER_LINEAR)
        assert want.shape == (H, W) and np.array_equal(planes[k], want), (k, int((planes[k] != want).sum()))
        assert mn[:, k].min() == planes[k].min() and mx[:, k].max() == planes[k].max(), k
        exact, cap = math.fsum(planes[k].reshape(-1).tolist()), 1e-9 * float(np.abs(planes[k].astype(np.float64)).sum())
        got = math.fsum(sm[:, k].tolist())
        print(f"{hw}->{HW} plane {k}: {mn.shape[0]} records, |sum - fsum| {abs(got - exact):.3e} (cap {cap:.3e})")
        assert abs(got - exact) <= cap, (k, got, exact)
    if (h, w) == (H, W):
        assert np.array_equal(planes, small)  # the same size copies


def test_a_misaligned_output_takes_the_scalar_path_with_identical_bytes():
    small = _small_planes(6, 6, seed=5)
    a = _planes_up(small, 64, 64)
    b = _planes_up(small, 64, 64, offset=4)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].min(0), b[1].min(0)) and np.array_equal(a[2].max(0), b[2].max(0))
    assert np.allclose(a[3].sum(0), b[3].sum(0), rtol=1e-12, atol=0)


# ---------------------------------------------------------------- 2. argument errors ---------------------------------------------
def test_bad_arguments_return_invalid_and_name_the_function():
    from animal_vision_amd._lib import AVX_ERR_INVALID, AVX_OK, lib
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    h, w, H, W = 6, 6, 64, 64
    d_in, d_out, d_part = ctx.malloc(3 * h * w * 4), ctx.malloc(3 * H * W * 4), ctx.malloc(8 * _cus() * 3 * 16)
    ctx.memset(d_in, 0)
    n = ctypes.c_int(0)

    def call(src=d_in.ptr, hh=h, ww=w, dst=d_out.ptr, HH=H, WW=W, part=d_part.ptr, np_=ctypes.byref(n)):
        return lib.avx_catch_planes_up(ctx._h, src, hh, ww, dst, HH, WW, part, np_, ctx.stream)

    try:
        bad = {
            "planes_small NULL": dict(src=None), "planes_out NULL": dict(dst=None), "partials_out NULL": dict(part=None), "n_partials NULL": dict(np_=None),
            "h = 0": dict(hh=0), "w < 0": dict(ww=-1), "H = 0": dict(HH=0), "W = 0": dict(WW=0),
            "h > H": dict(hh=H + 1), "w > W": dict(ww=W + 1),
            "out over in": dict(dst=d_in.ptr), "in inside out": dict(src=d_out.ptr + 3 * H * W * 4 - 3 * h * w * 4),
            "partials inside out": dict(part=d_out.ptr + 256), "partials over in": dict(part=d_in.ptr),
            "partials off by 8": dict(part=d_part.ptr + 8), "partials off by 4": dict(part=d_part.ptr + 4),
        }
        for name, kw in bad.items():
            assert call(**kw) == AVX_ERR_INVALID, name
            assert lib.avx_last_error(ctx._h).decode().startswith("avx_catch_planes_up"), (name, lib.avx_last_error(ctx._h))
        assert call() == AVX_OK and n.value >= 1
        ctx.sync()
    finally:
        for b in (d_in, d_out, d_part):
            b.free()


# ---------------------------------------------------------------- 3. the route against existing entry points --------------------
@pytest.fixture(scope="module")
def composed_planes(pred):
    """(hw, scale) -> (frame, the (H, W, 3) float32 catches): uint8 INTER_AREA resize -> the network's catches on the reduced frame ->
    avx_resize_hwc per plane.  Entry points that existed before the reduced route only; computed once per case."""
    import torch

    from animal_vision_amd import geometry, uv
    from animal_vision_amd.animals import HoneyBee
    from animal_vision_amd.ml.predict import pad_amounts

    cache = {}

    def get(hw, scale):
        if (hw, scale) not in cache:
            H, W = hw
            h, w = max(1, int(round(H * scale))), max(1, int(round(W * scale)))
            frame = _frame(hw)
            small = geometry.resize(frame, (w, h), geometry.INTER_AREA)
            assert small.shape == (h, w, 3) and small.dtype == np.uint8
            op32 = HoneyBee()._operator().padded_clone(32)
            dev = torch.from_numpy(small).to(pred.device)
            if pred.model.can_fuse_spectral():
                catches = pred.model.forward_from_u8(dev, pad_amounts(h, w, pred.stride), spectral=op32.weights)[0].cpu().numpy()
            else:
                catches = uv.spectral_integrate(pred.predict_device_nhwc(dev).cpu().numpy(), op32.weights)
            up = np.stack([geometry.resize(np.ascontiguousarray(catches[k]), (W, H), geometry.INTER_LINEAR) for k in range(3)], axis=-1)
            cache[(hw, scale)] = (frame, np.ascontiguousarray(up))
        return cache[(hw, scale)]

    return get


def _identity_tail(bee):
    """The bee's tail fed catches as a 3-band cube with identity weights, built as HoneyBee._visualize_staged builds it."""
    from animal_vision_amd.uv import HoneybeeOp

    tail = HoneybeeOp(lambdas=bee.lambdas, illuminant=bee.E, curves=(bee.UV_curve, bee.Blue_curve, bee.Green_curve), reflectance=bee.assume_hsi_is_reflectance,
                      adaptation=bee.adaptation, mapping_mode=bee.mapping_mode, custom_matrix=bee.custom_matrix, blur_sigma_px=bee.blur_sigma_px, eps=bee._eps)
    tail.weights = np.eye(3, dtype=np.float32)
    tail.desc.bands = 3
    tail.desc.weights_host = tail.weights.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    return tail


@pytest.mark.parametrize("hw,scale", CASES)
@pytest.mark.parametrize("mapping,adaptation,sigma", SETTINGS)
def test_route_equals_the_composition_of_existing_entry_points(pred, composed_planes, mapping, adaptation, sigma, hw, scale):
    """Identical bytes where the tail's statistics are order statistics (white patch: a maximum; none); gray world divides by a mean whose
    double partial sums are grouped differently: +-1 code, fewer than 1e-3 of the samples."""
    frame, planes = composed_planes(hw, scale)
    bee = _bee(pred, mapping, adaptation, sigma, scale)
    base, out = bee.visualize(frame)
    assert base is frame and out.shape == frame.shape and out.dtype == np.uint8
    want = _identity_tail(bee)(frame, hsi=planes, hsi_layout="nhwc")
    if adaptation == "gray_world":
        d = np.abs(out.astype(np.int16) - want.astype(np.int16))
        print("gray_world: max code difference", int(d.max()), "share", float((d > 0).mean()))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, (int(d.max()), float((d > 0).mean()))
    else:
        assert np.array_equal(out, want), int((out != want).sum())


def test_the_flag_is_no_longer_ignored(pred):
    frame = _frame((72, 88))
    full = _bee(pred).visualize(frame)[1]
    assert not np.array_equal(_bee(pred, scale=0.5).visualize(frame)[1], full)
    assert np.array_equal(_bee(pred, scale=1.0).visualize(frame)[1], full)  # outside [0.05, 1): the full-size route, as for the analytic converter


# ---------------------------------------------------------------- 4. the route against the CPU oracle ----------------------------
@pytest.fixture(scope="module")
def oracle_planes(pred, oracle):
    """(hw, scale) -> (frame, U, B, G at H x W): the oracle's resize of the oracle's catches of the network's cube of the oracle-reduced frame."""
    cache = {}

    def get(hw, scale):
        if (hw, scale) not in cache:
            H, W = hw
            h, w = max(1, int(round(H * scale))), max(1, int(round(W * scale)))
            frame = _frame(hw)
            small = oracle.cv_resize(frame, (w, h), oracle.INTER_AREA)
            assert small.dtype == np.uint8 and small.shape == (h, w, 3)
            ubg = oracle.honeybee_catches(pred.predict(small), LAM)
            cache[(hw, scale)] = (frame,) + tuple(oracle.cv_resize(np.ascontiguousarray(p, dtype=np.float32), (W, H), oracle.INTER_LINEAR) for p in ubg)
        return cache[(hw, scale)]

    return get


@pytest.mark.parametrize("hw,scale", CASES)
@pytest.mark.parametrize("adaptation", ["white_patch", "gray_world"])
def test_route_matches_the_oracle_chain(pred, oracle, oracle_planes, adaptation, hw, scale):
    frame, U, B, G = oracle_planes(hw, scale)
    _, out = _bee(pred, adaptation=adaptation, scale=scale).visualize(frame)
    want, _ = oracle.honeybee_tail(U, B, G, np.uint8, adaptation=adaptation, mapping_mode="opponent", blur_sigma_px=0.2, custom_matrix=CUSTOM)
    _bee_close(out, want)


# ---------------------------------------------------------------- 5. a reduced frame too small to pad ---------------------------
def test_a_too_small_reduced_frame_is_refused_before_any_launch(pred, monkeypatch):
    from animal_vision_amd.ml import MstHoneybeeStreamOp
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    def launched(*a, **kw):
        raise AssertionError("a launch was enqueued before the refusal")

    monkeypatch.setattr(pred, "_prepared", False)  # the operator's prepare() would run a probe frame: it must not get that far
    monkeypatch.setattr(_AVX, "conv_in_u8", launched)
    monkeypatch.setattr(pred, "predict_device_nhwc", launched)
    monkeypatch.setattr(pred, "honeybee_device", launched)
    bee = _bee(pred, scale=0.1)
    with pytest.raises(ValueError, match=r"37x45.*4x4"):
        bee.visualize(_frame((37, 45)))
    with pytest.raises(ValueError, match=r"hsi_scale"):
        MstHoneybeeStreamOp(pred, bee._operator(), 37, 45, depth=3, hsi_scale=0.1)


# ---------------------------------------------------------------- 6. the stream operator ----------------------------------------
def _through_pipeline(op, frames, H, W, batch):
    from animal_vision_amd.pipeline import FramePipeline

    got = {}
    pipe = FramePipeline(op, H, W, depth=3, batch=batch)
    pipe.run(((i, f) for i, f in enumerate(frames)), lambda i, o: got.__setitem__(i, o))
    pipe.close()
    assert sorted(got) == list(range(len(frames)))
    return [got[i] for i in range(len(frames))]


@pytest.fixture(scope="module")
def stream_frames():
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    return [structured_frame(40 + i, 72, 88) if i % 2 else noise_frame(40 + i, 72, 88) for i in range(5)]


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("setting", [("opponent", "gray_world", 0.2), ("falsecolor_uv_mixed", "white_patch", 1.0)])
def test_stream_op_equals_visualize(pred, stream_frames, setting, batch):
    """A fused-tail and a cube-tail setting, 5 frames at depth 3 (the last slot of batch 2 carries one frame): byte-identical to visualize."""
    from animal_vision_amd.ml import MstHoneybeeStreamOp

    bee = _bee(pred, *setting, scale=0.5)
    assert bee._operator().takes_catches() == (setting[0] == "opponent")
    op = MstHoneybeeStreamOp(pred, bee._operator(), 72, 88, depth=3, hsi_scale=0.5, batch=batch)
    assert op.max_batch == batch
    got = _through_pipeline(op, stream_frames, 72, 88, batch)
    for i, f in enumerate(stream_frames):
        assert np.array_equal(got[i], bee.visualize(f)[1]), i


def test_stream_op_without_a_scale_is_the_full_size_route(pred, stream_frames):
    from animal_vision_amd.ml import MstHoneybeeStreamOp

    bee = _bee(pred)._operator()
    op = MstHoneybeeStreamOp(pred, bee, 72, 88, depth=3)
    assert op.max_batch == 1
    got = _through_pipeline(op, stream_frames, 72, 88, 1)
    for i, f in enumerate(stream_frames):
        assert np.array_equal(got[i], pred.honeybee(f, bee)), i


# ---------------------------------------------------------------- 7. the command -----------------------------------------------
def _synthetic(spec):
    from animal_vision_amd.renderers import VideoRenderer

    vr = VideoRenderer(read_path=spec)
    vr.open()
    frames = []
    while True:
        f = vr.get_image()
        if f is None:
            break
        frames.append(f)
    vr.close()
    return frames


@pytest.mark.parametrize("extra", [[], ["--hsi-scale", "0.5"]])
def test_command_equals_visualize_and_split_batches_agree(tmp_path, capsys, extra):
    from animal_vision_amd.renderers import split_compose
    from animal_vision_amd.video import main, make_animal, parse_args, route

    src = "synthetic:96x64:5"
    argv = ["--species", "HoneyBee", "--hsi-model", "seeded"] + extra
    frames = _synthetic(src)
    assert len(frames) == 5 and frames[0].shape == (64, 96, 3)
    bee = make_animal(parse_args([src, "x.npy"] + argv))
    assert route(bee) == "honeybee_mst" and bee.hsi_downsample == bool(extra)
    want = [bee.visualize(f)[1] for f in frames]
    plain, split1, split2 = (str(tmp_path / n) for n in ("plain.npy", "split1.npy", "split2.npy"))
    assert main([src, plain] + argv) == 0
    assert "5 frames" in capsys.readouterr().err
    assert np.array_equal(np.load(plain), np.stack(want))
    assert main([src, split1] + argv + ["--split-compare"]) == 0
    assert main([src, split2] + argv + ["--split-compare", "--batch", "2"]) == 0
    capsys.readouterr()
    got1, got2 = np.load(split1), np.load(split2)
    assert np.array_equal(got1, got2)
    for k, f in enumerate(frames):
        assert np.array_equal(got2[k], split_compose(f, want[k], left_label="Original", right_label="Transformed")), k
        labelled = split_compose(f, f, left_label="Original", right_label="Transformed")  # the input under the same labels (their box dims what it covers)
        assert np.array_equal(got2[k][:, :48], labelled[:, :48]), k                       # the left half is the input's, whatever the right half holds
        assert np.array_equal(got2[k][48:, :40], f[48:, :40]), k                          # and below the label box the input's bytes themselves


def test_command_raw_nv12_scaled_into_a_yuv_file(tmp_path, capsys):
    from animal_vision_amd import yuv
    from animal_vision_amd.synthetic import structured_frame
    from animal_vision_amd.video import main, make_animal, parse_args

    H, W, Hd, Wd, fmt = 64, 96, 32, 48, "nv12"
    payloads = yuv.rgb_to_yuv(np.stack([structured_frame(70 + i, H, W) for i in range(3)]), pix_fmt=fmt)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "bee.yuv")
    payloads.tofile(src)
    argv = ["--species", "HoneyBee", "--pix-fmt", fmt, "--size", f"{W}x{H}", "--scale", f"{Wd}x{Hd}", "--hsi-model", "seeded"]
    assert main([src, dst] + argv) == 0
    assert "3 frames" in capsys.readouterr().err
    got = np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(3, -1)
    assert got.shape[1] == yuv.frame_size(fmt, Hd, Wd)
    bee = make_animal(parse_args([src, dst] + argv))
    small = yuv.yuv_to_rgb_scaled(payloads, H, W, Hd, Wd, pix_fmt=fmt)
    for k in range(3):
        assert np.array_equal(got[k], yuv.rgb_to_yuv(bee.visualize(small[k])[1], pix_fmt=fmt)), k
