"""GPU: Cat through the frame pipeline.

  * avx_cat_wide_u8 (csrc/cat_wide.hip, one fused launch per batch) against the chain that defines it, frame by frame:
    avx_binocular_warp_u8 -> float32 frame -> avx_dichromat_u8(in_f32 = 1).  Identical bytes.
  * avx_center_zoom_u8 against geometry.center_zoom (avx_resize_hwc of the contiguous crop).  Identical bytes.
  * both against what lies outside the project's device code: the reference's goldens and oracle.cat_visualize.
  * CatStreamOp through FramePipeline, and the `video` command, against Cat().visualize + split_compose.
  * the refusals of the two entry points, and their ordering on a stream without synchronisation."""
import ctypes

import numpy as np
import pytest

import _yuv_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

# (H, W): smaller than the halo both ways; odd; several ragged 32 x 16 tiles both ways; an exact multiple of the tile (and of
# 32 x 32); that plus one; one video frame
SIZES = [(6, 5), (37, 53), (70, 131), (96, 160), (97, 161), (1080, 1920)]


@pytest.fixture(scope="module")
def G():
    from animal_vision_amd import geometry

    return geometry


@pytest.fixture(scope="module")
def ctx():
    from animal_vision_amd.runtime import get_context

    return get_context()


def _cat(**attrs):
    """A Cat with other class constants (FOV, SPEC): a subclass, as a user would write it."""
    from animal_vision_amd.animals import Cat

    return type("CatVariant", (Cat,), attrs)() if attrs else Cat()


def _spec(**kw):
    from animal_vision_amd.dichromat import DichromatSpec

    base = dict(alpha=0.5, s_scale=1.0, color="cat_merge", sigma=1.0)
    base.update(kw)
    return DichromatSpec("cat", **base)


def _tables(G, cat, H, W):
    return G.binocular_warp_tables(H, W, W, H, cat.CAMERA_HFOV_DEG, cat.CAT_PER_EYE_HALF_FOV_DEG, cat.CAT_OVERLAP_DEG)


def _noise(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _chain(G, ctx, frames, cat):
    """The definition: per frame avx_binocular_warp_u8 into a float32 frame, then avx_dichromat_u8 with in_f32 = 1."""
    from animal_vision_amd.dichromat import DichromatOp

    n, H, W, _ = frames.shape
    op = DichromatOp(cat.SPEC, ctx)
    tables = _tables(G, cat, H, W)
    d_in, d_warp, d_out = ctx.malloc(H * W * 3), ctx.malloc(H * W * 3 * 4), ctx.malloc(H * W * 3)
    out = np.empty_like(frames)
    try:
        op.desc.in_f32 = 1
        for f in range(n):
            ctx.upload(frames[f], d_in)
            G.binocular_warp_device(ctx, d_in, H, W, tables, H, W, d_warp)
            op.run_device(d_warp, d_out, 1, H, W)
            out[f] = ctx.download(d_out, (H, W, 3), np.uint8)
    finally:
        d_in.free(); d_warp.free(); d_out.free()
    return out


def _fused(G, ctx, frames, cat, capacity=None):
    """avx_cat_wide_u8 over the first len(frames) frames of buffers that hold `capacity`; returns the whole output buffer."""
    from animal_vision_amd.dichromat import DichromatOp

    n, H, W, _ = frames.shape
    cap = capacity or n
    op = DichromatOp(cat.SPEC, ctx)
    tab, ptrs = G.binocular_warp_tables_device(ctx, _tables(G, cat, H, W))
    host = np.full((cap, H, W, 3), 0xA5, np.uint8)
    host[:n] = frames
    d_in, d_out = ctx.upload(host), ctx.upload(np.full((cap, H, W, 3), 0x5A, np.uint8))
    try:
        G.cat_wide_device(ctx, d_in, d_out, n, H, W, op.desc, ptrs)
        return ctx.download(d_out, (cap, H, W, 3), np.uint8)
    finally:
        d_in.free(); d_out.free(); tab.free()


def _same(got, want, what):
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]])


# ---------------------------------------------------------------- the fused kernel against the chain -----------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_wide_view_equals_the_chain(G, ctx, H, W):
    frames = _noise(H + W, 1, H, W, 3)
    _same(_fused(G, ctx, frames, _cat()), _chain(G, ctx, frames, _cat()), (H, W))


def test_wide_view_of_structured_content_equals_the_chain(G, ctx):
    from animal_vision_amd.synthetic import structured_frame

    frames = np.stack([structured_frame(5, 70, 131), structured_frame(6, 70, 131)])
    _same(_fused(G, ctx, frames, _cat()), _chain(G, ctx, frames, _cat()), "structured")


def test_dark_frame_and_per_frame_flags(G, ctx):
    """A frame whose bytes are all 0 or 1 is not divided by 255 (get_normalized_image); in a batch that is decided frame by frame."""
    H, W = 70, 131
    dark = _noise(1, H, W, 3) & 1
    bright = _noise(2, 2, H, W, 3)
    batch = np.stack([bright[0], dark, bright[1]])
    want = _chain(G, ctx, batch, _cat())
    assert want[1].max() > 2  # a 1 is 1.0 here; divided by 255 it would be 3e-4 linear, which no sum of the tail lifts above code 2
    _same(_fused(G, ctx, batch[1:2], _cat()), want[1:2], "dark alone")
    _same(_fused(G, ctx, batch, _cat()), want, "bright, dark, bright")
    _same(_fused(G, ctx, batch[::-1][:2].copy(), _cat()), want[::-1][:2], "bright, dark")
    almost = dark.copy()
    almost[H - 1, W - 1, 2] = 2  # one byte above 1, the frame's last: the whole frame is divided
    _same(_fused(G, ctx, almost[None], _cat()), _chain(G, ctx, almost[None], _cat()), "one byte above 1")


def test_fewer_frames_than_the_buffers_hold(G, ctx):
    H, W = 37, 53
    frames = _noise(7, 2, H, W, 3)
    got = _fused(G, ctx, frames, _cat(), capacity=4)
    _same(got[:2], _chain(G, ctx, frames, _cat()), "n = 2 of 4")
    assert (got[2:] == 0x5A).all()  # the frames beyond n_frames are not written


@pytest.mark.parametrize("H,W", [(6, 5), (70, 131)])
@pytest.mark.parametrize("spec", [dict(post="none"), dict(sigma=1.7), dict(sigma=0.4), dict(alpha=0.3)], ids=["r0", "ksize15", "ksize5", "alpha"])
def test_other_tails_through_a_subclass(G, ctx, spec, H, W):
    from animal_vision_amd.dichromat import cv_auto_ksize

    cat = _cat(SPEC=_spec(**spec))
    if "sigma" in spec:
        assert cv_auto_ksize(spec["sigma"]) == {1.7: 15, 0.4: 5}[spec["sigma"]]
    frames = _noise(11, 2, H, W, 3)
    _same(_fused(G, ctx, frames, cat), _chain(G, ctx, frames, cat), (spec, H, W))


@pytest.mark.parametrize("fov,band", [(dict(CAMERA_HFOV_DEG=60.0, CAT_PER_EYE_HALF_FOV_DEG=100.0, CAT_OVERLAP_DEG=20.0), True),
                                      (dict(CAMERA_HFOV_DEG=170.0, CAT_PER_EYE_HALF_FOV_DEG=60.0, CAT_OVERLAP_DEG=90.0), False)],
                         ids=["narrow-camera", "all-overlap"])
def test_other_fov_constants_through_a_subclass(G, ctx, fov, band):
    """Where neither eye sees the camera (wL = wR = 0 over a band of columns) the output is the 1e-8 quotient of zeros."""
    H, W = 70, 131
    cat = _cat(**fov)
    _, _, _, wL, wR = _tables(G, cat, H, W)
    blind = (wL == 0) & (wR == 0)
    assert bool(blind[8:-8].any()) == band and not blind.all()
    frames = _noise(13, 2, H, W, 3)
    want = _chain(G, ctx, frames, cat)
    got = _fused(G, ctx, frames, cat)
    _same(got, want, fov)
    if band:
        inner = np.flatnonzero(blind)
        inner = inner[(inner >= inner.min() + 8) & (inner <= inner.max() - 8)]  # further than the blur radius from a seeing column
        assert inner.size and (got[:, :, inner] == 0).all()


# ---------------------------------------------------------------- the baseline -----------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_center_zoom_equals_geometry_center_zoom(G, ctx, H, W):
    from animal_vision_amd.animals._dichromats import CatStreamOp

    n = 1 if H > 500 else 3
    frames = _noise(H * W, n, H, W, 3)
    rect = CatStreamOp.crop_rect(_cat(), H, W)
    scale = G.zoom_scale_from_cat_ratio(camera_hfov_deg=100.0, cat_per_eye_half_fov_deg=105.0, cat_to_human_ratio=1.30)
    d_in, d_out = ctx.upload(frames), ctx.malloc(frames.nbytes)
    try:
        G.center_zoom_device(ctx, d_in, d_out, n, H, W, rect)
        got = ctx.download(d_out, frames.shape, np.uint8)
    finally:
        d_in.free(); d_out.free()
    for f in range(n):
        _same(got[f], G.center_zoom(frames[f], scale), (H, W, f))


@pytest.mark.parametrize("rect", [(17, 9, 1, 1), (0, 0, 1, 1), (52, 36, 1, 1), (0, 5, 53, 1), (30, 0, 1, 37), (0, 0, 53, 37), (3, 2, 50, 35)])
def test_center_zoom_of_any_crop_inside_the_frame(G, ctx, rect):
    """A crop of one pixel, of one row, of one column, the whole frame: cv2.resize(frame[y0:y0+ch, x0:x0+cw], (W, H))."""
    H, W = 37, 53
    x0, y0, cw, ch = rect
    frames = _noise(sum(rect), 2, H, W, 3)
    d_in, d_out = ctx.upload(frames), ctx.malloc(frames.nbytes)
    try:
        G.center_zoom_device(ctx, d_in, d_out, 2, H, W, rect)
        got = ctx.download(d_out, frames.shape, np.uint8)
    finally:
        d_in.free(); d_out.free()
    for f in range(2):
        _same(got[f], G.resize(np.ascontiguousarray(frames[f, y0:y0 + ch, x0:x0 + cw]), (W, H), G.INTER_LINEAR), (rect, f))


# ---------------------------------------------------------------- anchors outside the project's device code ------------------------
def test_baseline_against_the_reference_goldens(G, ctx):
    from animal_vision_amd.animals._dichromats import CatStreamOp

    g = load_golden("geometry")
    for k in ("n48", "s60"):
        f = g[f"in_{k}"]
        H, W = f.shape[:2]
        op = CatStreamOp(_cat(), H, W, depth=1, batch=2, ctx=ctx)
        try:
            d_in, d_out = op.slot_buffers(0)
            ctx.upload(np.stack([f, f[::-1]]), d_in)
            op.run_device(d_in, d_out, 2, H, W)
            base = ctx.download(op.slot_baseline(0), (2, H, W, 3), np.uint8)
        finally:
            op.close()
        assert np.array_equal(base[0], g[f"cat_human_{k}"]), k
        assert np.array_equal(base[1], G.center_zoom(np.ascontiguousarray(f[::-1]), float(g["zoom_scale"]))), k


def test_wide_view_against_the_oracle(G, ctx, oracle):
    """The criterion tests/test_geometry_gpu.py::test_full_cat_vs_reference_golden holds the chain to, on its inputs: within one
    code (the decode of the warped float sample is the device powf), fewer than 5e-3 of the samples off."""
    frame = _noise(3, 270, 480, 3)  # rng(3), 270 x 480: that test's frame
    want_h, want_c = oracle.cat_visualize(frame)
    got = _fused(G, ctx, frame[None], _cat())[0]
    d = np.abs(got.astype(np.int16) - want_c.astype(np.int16))
    print("oracle: max diff", int(d.max()), "share", float((d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() < 5e-3, (int(d.max()), float((d > 0).mean()))
    g = load_golden("geometry")
    for k in ("n48", "s60"):
        got = _fused(G, ctx, g[f"in_{k}"][None], _cat())[0]
        d = np.abs(got.astype(np.int16) - g[f"cat_out_{k}"].astype(np.int16))
        assert d.max() <= 1 and (d > 0).mean() < 5e-3, (k, int(d.max()), float((d > 0).mean()))


# ---------------------------------------------------------------- the stream --------------------------------------------------------
@pytest.fixture(scope="module")
def stream_frames():
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    return [structured_frame(20 + i, 96, 160) if i % 2 else noise_frame(20 + i, 96, 160) for i in range(7)]


def _through_pipeline(op, frames, H, W, **kw):
    from animal_vision_amd.pipeline import FramePipeline

    pipe = FramePipeline(op, H, W, **kw)
    got = {}
    try:
        st = pipe.run(iter(enumerate(frames)), lambda i, o: got.__setitem__(i, o.copy()))
    finally:
        pipe.close()
    assert st.frames == len(frames) and sorted(got) == list(range(len(frames)))
    return [got[i] for i in range(len(frames))]


@pytest.fixture(scope="module")
def visualized(stream_frames):
    """Cat().visualize of the stream's frames, once: (baseline, wide view) pairs."""
    cat = _cat()
    return [cat.visualize(f) for f in stream_frames]


def test_visualize_is_the_chain_and_the_zoom(G, ctx, stream_frames, visualized):
    f = stream_frames[0]
    scale = G.zoom_scale_from_cat_ratio(camera_hfov_deg=100.0, cat_per_eye_half_fov_deg=105.0, cat_to_human_ratio=1.30)
    _same(visualized[0][0], G.center_zoom(f, scale), "baseline")
    _same(visualized[0][1], _chain(G, ctx, f[None], _cat())[0], "wide view")


def test_visualize_keeps_at_most_four_sizes(ctx):
    cat = _cat()
    for k in range(6):
        base, out = cat.visualize(_noise(k, 8 + k, 12, 3))
        assert base.shape == out.shape == (8 + k, 12, 3)
    assert len(cat._u8_plans) == 4 and {key[0] for key in cat._u8_plans} == {10, 11, 12, 13}


@pytest.mark.parametrize("io_format", ["rgb", "i420"])
def test_stream_equals_visualize_and_split_compose(ctx, stream_frames, visualized, io_format):
    """7 frames, depth 2, batch 3: two full slots and a partial one, the split frame composed against the zoomed baseline."""
    from animal_vision_amd.animals._dichromats import CatStreamOp
    from animal_vision_amd.renderers import split_compose

    H, W = 96, 160
    op = CatStreamOp(_cat(), H, W, depth=2, batch=3, ctx=ctx)
    assert op.max_batch == 3 and op.slot_baseline(0) is not op.slot_buffers(0)[0]
    try:
        if io_format == "rgb":
            got = _through_pipeline(op, stream_frames, H, W, depth=2, split_compare=True, split_baseline=True, batch=3)
            pairs = visualized
        else:
            payloads = R.encode(np.stack(stream_frames))
            got = _through_pipeline(op, list(payloads), H, W, depth=2, split_compare=True, split_baseline=True, batch=3, io_format="i420")
            cat = _cat()
            pairs = [cat.visualize(f) for f in R.decode(payloads, H, W)]
    finally:
        op.close()
    for k, (base, out) in enumerate(pairs):
        want = split_compose(base, out, left_label="Original", right_label="Transformed")
        _same(got[k], want if io_format == "rgb" else R.encode(want), (io_format, k))


def test_stream_without_the_warp_is_the_dichromat_kernel(ctx, stream_frames):
    from animal_vision_amd.animals import Cat
    from animal_vision_amd.animals._dichromats import CatStreamOp
    from animal_vision_amd.dichromat import DichromatOp

    H, W = 96, 160
    cat = _cat(ENABLE_FOV_WARP=False)
    op = CatStreamOp(cat, H, W, depth=2, batch=3, ctx=ctx)
    try:
        got = _through_pipeline(op, stream_frames, H, W, depth=2, batch=3)
    finally:
        op.close()
    want = DichromatOp(Cat.SPEC, ctx)(np.stack(stream_frames))
    for k in range(len(stream_frames)):
        _same(got[k], want[k], k)
    base, out = cat.visualize(stream_frames[1])
    _same(out, want[1], "visualize without the warp")


def test_stream_at_a_zoom_scale_below_one_lends_the_input_as_baseline(ctx, stream_frames):
    """A camera wider than 180 degrees has a negative tangent: zoom_scale_from_cat_ratio is below 1, center_zoom returns the frame
    itself, and the op's baseline is the slot's input -- no zoom launch, no baseline buffer."""
    from animal_vision_amd.animals._dichromats import CatStreamOp
    from animal_vision_amd.renderers import split_compose

    H, W = 96, 160
    cat = _cat(CAMERA_HFOV_DEG=200.0)
    assert CatStreamOp.crop_rect(cat, H, W) is None
    op = CatStreamOp(cat, H, W, depth=2, batch=2, ctx=ctx)
    try:
        assert op.slot_baseline(1) is op.slot_buffers(1)[0] and op._base == [None, None]
        got = _through_pipeline(op, stream_frames[:3], H, W, depth=2, split_compare=True, split_baseline=True, batch=2)
    finally:
        op.close()
    for k, f in enumerate(stream_frames[:3]):
        base, out = cat.visualize(f)
        assert base is f
        _same(got[k], split_compose(f, out, left_label="Original", right_label="Transformed"), k)


def test_a_pipeline_batch_beyond_the_ops_is_refused(ctx):
    from animal_vision_amd.animals._dichromats import CatStreamOp
    from animal_vision_amd.pipeline import FramePipeline

    op = CatStreamOp(_cat(), 32, 48, depth=2, batch=2, ctx=ctx)
    try:
        with pytest.raises(ValueError, match="at most 2"):
            FramePipeline(op, 32, 48, depth=2, batch=4, split_compare=True, split_baseline=True)
    finally:
        op.close()
    with pytest.raises(ValueError):
        CatStreamOp(_cat(), 32, 48, depth=2, batch=0, ctx=ctx)


# ---------------------------------------------------------------- the command ------------------------------------------------------
def _read_y4m(path):
    from animal_vision_amd.renderers.y4m import Y4MReader

    rd = Y4MReader(path)
    out = []
    while (f := rd.read()) is not None:
        out.append(f)
    rd.close()
    return out


def test_command_y4m_split_compare_batches_agree_with_visualize(tmp_path, capsys, stream_frames):
    from animal_vision_amd.renderers import split_compose
    from animal_vision_amd.video import main, make_animal, parse_args, stream_op

    H, W = 96, 160
    payloads = R.encode(np.stack(stream_frames))
    src = str(tmp_path / "in.y4m")
    with open(src, "wb") as f:
        f.write(R.y4m_bytes(list(payloads), H, W, header="F25:1 Ip A1:1 C420jpeg XYSCSS=420JPEG"))
    one, four = str(tmp_path / "b1.y4m"), str(tmp_path / "b4.y4m")
    assert main([src, one, "--species", "Cat", "--split-compare"]) == 0
    assert "7 frames" in capsys.readouterr().err
    assert main([src, four, "--species", "Cat", "--split-compare", "--batch", "4", "--depth", "2"]) == 0
    assert "7 frames" in capsys.readouterr().err
    assert open(one, "rb").read() == open(four, "rb").read()
    frames = _read_y4m(four)
    assert len(frames) == 7
    cat = make_animal(parse_args([src, four, "--species", "Cat"]))
    for k, rgb in enumerate(R.decode(payloads, H, W)):
        base, out = cat.visualize(rgb)
        assert not np.array_equal(base, rgb)  # the left half is the zoomed baseline, not the input
        _same(frames[k], R.encode(split_compose(base, out, left_label="Original", right_label="Transformed")), k)
    op = stream_op(cat, H, W, 3, 4)
    try:
        assert type(op).__name__ == "CatStreamOp" and op.max_batch == 4 and len(op._bufs) == 3
    finally:
        op.close()


def test_command_raw_nv12_scaled(tmp_path, capsys):
    from animal_vision_amd import yuv
    from animal_vision_amd.synthetic import structured_frame
    from animal_vision_amd.video import main

    H, W, Hd, Wd, fmt = 96, 160, 48, 80, "nv12"
    payloads = yuv.rgb_to_yuv(np.stack([structured_frame(70 + i, H, W) for i in range(3)]), pix_fmt=fmt)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "cat.yuv")
    payloads.tofile(src)
    assert main([src, dst, "--species", "Cat", "--pix-fmt", fmt, "--size", f"{W}x{H}", "--scale", f"{Wd}x{Hd}", "--batch", "2"]) == 0
    assert "3 frames" in capsys.readouterr().err
    got = np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(3, -1)
    assert got.shape[1] == yuv.frame_size(fmt, Hd, Wd)
    small = yuv.yuv_to_rgb_scaled(payloads, H, W, Hd, Wd, pix_fmt=fmt)
    cat = _cat()
    for k in range(3):
        _same(got[k], yuv.rgb_to_yuv(cat.visualize(small[k])[1], pix_fmt=fmt), k)


# ---------------------------------------------------------------- refusals ---------------------------------------------------------
def _err(ctx):
    from animal_vision_amd._lib import lib

    return lib.avx_last_error(ctx._h).decode()


def test_cat_wide_refusals(G, ctx):
    from animal_vision_amd._lib import AVX_COLOR_MATRIX, AVX_ERR_INVALID, AVX_OK, AVX_POST_ROWGAIN, AVX_POST_STREAK, DichromatDesc, lib
    from animal_vision_amd.dichromat import DichromatOp

    H, W = 16, 24
    op = DichromatOp(_cat().SPEC, ctx)
    tab, ptrs = G.binocular_warp_tables_device(ctx, _tables(G, _cat(), H, W))
    d_in, d_out = ctx.upload(_noise(0, H, W, 3)), ctx.upload(np.full((H, W, 3), 0x5A, np.uint8))

    def call(inp=d_in.ptr, out=d_out.ptr, n=1, h=H, w=W, desc=op.desc, tables=None, null_desc=False):
        t = list(ptrs if tables is None else tables)
        return lib.avx_cat_wide_u8(ctx._h, inp, out, n, h, w, None if null_desc else ctypes.byref(desc), *t, ctx.stream)

    def desc_with(**kw):
        d = DichromatDesc.from_buffer_copy(bytes(op.desc))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    try:
        bad = [dict(inp=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(h=-3), dict(null_desc=True),
               dict(desc=desc_with(struct_size=ctypes.sizeof(DichromatDesc) - 4)), dict(desc=desc_with(color_mode=AVX_COLOR_MATRIX)),
               dict(desc=desc_with(post_mode=AVX_POST_ROWGAIN)), dict(desc=desc_with(post_mode=AVX_POST_STREAK)), dict(desc=desc_with(post_mode=7)),
               dict(desc=desc_with(ksize=0)), dict(desc=desc_with(ksize=8)), dict(desc=desc_with(ksize=35)), dict(desc=desc_with(ksize=-9))]
        bad += [dict(tables=[None if j == i else p for j, p in enumerate(ptrs)]) for i in range(5)]
        for kw in bad:
            assert call(**kw) == AVX_ERR_INVALID, kw
            assert _err(ctx).startswith("avx_cat_wide_u8:"), (kw, _err(ctx))
        assert call(n=0) == AVX_OK
        ctx.sync()
        assert (ctx.download(d_out, (H, W, 3), np.uint8) == 0x5A).all()  # no refused call, nor n_frames == 0, wrote anything
        assert call(desc=desc_with(in_f32=1, variant=2)) == AVX_OK  # both ignored
        got = ctx.download(d_out, (H, W, 3), np.uint8)
        assert call() == AVX_OK
        assert np.array_equal(got, ctx.download(d_out, (H, W, 3), np.uint8))
    finally:
        d_in.free(); d_out.free(); tab.free()


def test_center_zoom_refusals(ctx):
    from animal_vision_amd._lib import AVX_ERR_INVALID, AVX_OK, lib

    H, W = 16, 24
    d_in, d_out = ctx.upload(_noise(0, H, W, 3)), ctx.upload(np.full((H, W, 3), 0x5A, np.uint8))

    def call(inp=d_in.ptr, out=d_out.ptr, n=1, h=H, w=W, rect=(4, 3, 12, 8)):
        return lib.avx_center_zoom_u8(ctx._h, inp, out, n, h, w, *rect, ctx.stream)

    try:
        bad = [dict(inp=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(w=-1),
               dict(rect=(4, 3, 0, 8)), dict(rect=(4, 3, 12, 0)), dict(rect=(4, 3, -2, 8)), dict(rect=(-1, 3, 12, 8)), dict(rect=(4, -1, 12, 8)),
               dict(rect=(13, 3, 12, 8)), dict(rect=(4, 9, 12, 8)), dict(rect=(0, 0, 25, 16)), dict(rect=(0, 0, 24, 17)),
               dict(rect=(2**31 - 1, 0, 2, 1)), dict(rect=(0, 0, 2**31 - 1, 1))]
        for kw in bad:
            assert call(**kw) == AVX_ERR_INVALID, kw
            assert _err(ctx).startswith("avx_center_zoom_u8:"), (kw, _err(ctx))
        assert call(n=0) == AVX_OK
        ctx.sync()
        assert (ctx.download(d_out, (H, W, 3), np.uint8) == 0x5A).all()
        assert call(rect=(12, 8, 12, 8)) == AVX_OK and call(rect=(0, 0, 24, 16)) == AVX_OK  # flush with the frame's far corner; the frame
        ctx.sync()
    finally:
        d_in.free(); d_out.free()


# ---------------------------------------------------------------- sequencing -------------------------------------------------------
def test_calls_are_ordered_on_a_stream_without_synchronisation(G, ctx):
    """h2d -> wide view -> zoom of that -> wide view of that -> d2h on one non-default stream, one synchronisation at the end: the
    entry points order themselves like kernels, with nothing left of the chain's per-call synchronisations to lean on."""
    from animal_vision_amd._lib import lib
    from animal_vision_amd.dichromat import DichromatOp

    H, W, n = 70, 131, 2
    cat = _cat()
    rect = (20, 10, 90, 50)
    op = DichromatOp(cat.SPEC, ctx)
    tab, ptrs = G.binocular_warp_tables_device(ctx, _tables(G, cat, H, W))
    frames, warm = _noise(21, n, H, W, 3), _noise(22, n, H, W, 3)
    nbytes = frames.nbytes
    s = ctx.stream_create()
    h_in, h_out = ctx.pinned(frames.shape, np.uint8), ctx.pinned(frames.shape, np.uint8)
    bufs = [ctx.malloc(nbytes) for _ in range(4)]

    def enqueue(src):
        h_in.array[...] = src
        ctx._check(lib.avx_memcpy_h2d(ctx._h, bufs[0].ptr, h_in.ptr, nbytes, s))
        G.cat_wide_device(ctx, bufs[0], bufs[1], n, H, W, op.desc, ptrs, s)
        G.center_zoom_device(ctx, bufs[1], bufs[2], n, H, W, rect, s)
        G.cat_wide_device(ctx, bufs[2], bufs[3], n, H, W, op.desc, ptrs, s)
        ctx._check(lib.avx_memcpy_d2h(ctx._h, h_out.ptr, bufs[3].ptr, nbytes, s))

    try:
        enqueue(warm)  # the warm-up: the stream's workspace and table cache take their size
        ctx.sync(s)
        enqueue(frames)
        ctx.sync(s)
        got = h_out.array.copy()
    finally:
        ctx.sync(s)
        ctx.stream_destroy(s)
        h_in.free(); h_out.free(); tab.free()
        for b in bufs:
            b.free()
    a = _chain(G, ctx, frames, cat)
    x0, y0, cw, ch = rect
    b = np.stack([G.resize(np.ascontiguousarray(a[f, y0:y0 + ch, x0:x0 + cw]), (W, H), G.INTER_LINEAR) for f in range(n)])
    _same(got, _chain(G, ctx, b, cat), "wide(zoom(wide(frames)))")
