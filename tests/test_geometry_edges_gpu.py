"""GPU: the kernels of csrc/geom.hip and csrc/resize_common.h at their edges, bit for bit against the oracle (oracle/cvref.cpp,
itself held to the float64 definitions by test_cvref_definition_host.py): degenerate sizes, every interpolation, the float4 branch
and pointers that forbid it, more items than one pass of the grid-stride loops covers, table-cache eviction, non-finite samples and
coordinates, and output sizes that differ from the input's.

GRID is the number of items all threads of a full launch cover before any of them goes round its loop again: 16 workgroups of
256 threads per compute unit (grid_for in geom.hip), 1,048,576 on the 256 compute units of an MI355X."""
import numpy as np
import pytest

import _geom_ref as R
from _geom_cases import EDGES, GPU_SUITE_F32, GPU_SUITE_U8, NONFINITE, REMAP_SIZES, SOBEL_SIZES, put_nonfinite, spanning_maps

pytestmark = pytest.mark.gpu

INTERPS = (R.INTER_NEAREST, R.INTER_LINEAR, R.INTER_CUBIC, R.INTER_AREA)


@pytest.fixture(scope="module")
def G():
    from animal_vision_amd import geometry

    return geometry


@pytest.fixture(scope="module")
def ctx():
    from animal_vision_amd.runtime import get_context

    return get_context()


@pytest.fixture(scope="module")
def GRID(ctx):
    return int(getattr(ctx, "num_cus", 256)) * 16 * 256


def _n(shape, dsize):
    return max(shape[0], shape[1], dsize[0], dsize[1])


# ---- 1. resize, float32 ------------------------------------------------------------------------------------------------------
OVER_GRID_F32 = [
    ((60, 84, 1), (1200, 1100)),    # 1,320,000 destination pixels: the per-pixel linear kernel goes round its loop
    ((60, 84, 3), (640, 600)),      # 1,152,000 destination elements: the per-element kernels (nearest, cubic) do
    ((1210, 1290, 1), (1100, 1000)),  # the same for the general INTER_AREA kernel ...
    ((2200, 2400, 1), (1200, 1100)),  # ... and for the integer-ratio one (2 x 2 blocks)
]
RESIZE_F32 = [c for c in GPU_SUITE_F32 + GPU_SUITE_U8 + EDGES if _n(*c) < 2999] + [
    ((33, 47, 4), (101, 77)), ((33, 47, 8), (101, 77)), ((33, 47, 8), (20, 11)),  # C % 4 == 0: the float4 branch of the linear kernel
] + OVER_GRID_F32


@pytest.mark.parametrize("shape,dsize", RESIZE_F32)
def test_resize_f32_edges_bit_exact_vs_oracle(G, oracle, GRID, shape, dsize):
    if (shape, dsize) in OVER_GRID_F32:
        assert dsize[0] * dsize[1] * shape[2] > GRID
    img = np.random.default_rng(sum(shape)).random(shape, dtype=np.float32)
    for interp in INTERPS:
        got = G.resize(img, dsize, interp)
        want = oracle.cv_resize(img, dsize, interp)
        assert np.array_equal(got, want), (shape, dsize, interp, float(np.abs(got - want).max()))


# ---- 2. float4 branch and alignment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dsize", [((45, 64, 4), (48, 27)), ((33, 47, 4), (101, 77)), ((7, 1, 4), (1, 3))])
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (4, 4), (4, 0), (0, 4)])
def test_resize_linear_c4_whole_and_misaligned_views(G, ctx, oracle, shape, dsize, src_off, dst_off):
    """INTER_LINEAR with C = 4 on buffers that allow 16-byte accesses and on views 4 bytes into a larger buffer, which do not."""
    (H, W, C), (Wd, Hd) = shape, dsize
    img = np.random.default_rng(sum(shape)).random(shape, dtype=np.float32)
    want = oracle.cv_resize(img, dsize, R.INTER_LINEAR)
    d_src, d_dst = ctx.malloc(img.nbytes + 16), ctx.malloc(want.nbytes + 16)
    try:
        assert d_src.ptr % 16 == 0 and d_dst.ptr % 16 == 0
        ctx.memset(d_dst, 0xFF)
        v_src, v_dst = d_src.view(src_off, img.nbytes), d_dst.view(dst_off, want.nbytes)
        ctx.upload(img, v_src)
        G.resize_device(ctx, v_src, np.float32, H, W, C, Hd, Wd, R.INTER_LINEAR, d_dst=v_dst)
        got = ctx.download(v_dst, want.shape, np.float32)
        whole = ctx.download(d_dst, (want.nbytes + 16,), np.uint8)
    finally:
        d_src.free()
        d_dst.free()
    assert np.array_equal(got, want), (shape, dsize, src_off, dst_off)
    assert (whole[:dst_off] == 0xFF).all() and (whole[dst_off + want.nbytes:] == 0xFF).all(), "bytes outside the destination view were written"


# ---- 3. resize, uint8 --------------------------------------------------------------------------------------------------------
RESIZE_U8 = [((64, 80, 3), (40, 32)),    # 2 x 2: (sum + 2) >> 2
             ((64, 80, 3), (20, 16)),    # 4 x 4
             ((9, 30, 3), (10, 9)),      # 3 x 1
             ((50, 70, 3), (17, 13)),    # general ratio
             ((50, 70, 3), (80, 40)),    # enlarging on one axis only: INTER_AREA runs as INTER_LINEAR
             ((1, 1, 3), (4, 3)),
             ((600, 640, 3), (213, 200)),
             ((1200, 1280, 3), (640, 600)),  # 1,152,000 destination elements (2 x 2 blocks): every uint8 kernel goes round its loop ...
             ((1210, 1290, 3), (640, 600))]  # ... the general-ratio one too


@pytest.mark.parametrize("shape,dsize", RESIZE_U8)
def test_resize_u8_linear_area_bit_exact_vs_oracle(G, oracle, GRID, shape, dsize):
    if shape[0] >= 1200:
        assert dsize[0] * dsize[1] * shape[2] > GRID
    frames = [np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)]
    if shape[0] < 600:
        frames += [np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)]
    for img in frames:
        for interp in (R.INTER_LINEAR, R.INTER_AREA):
            got = G.resize(img, dsize, interp)
            want = oracle.cv_resize(img, dsize, interp)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (shape, dsize, interp, int(img[0, 0, 0]),
                                                                         int(np.abs(got.astype(int) - want.astype(int)).max()))


# ---- 4. table cache ----------------------------------------------------------------------------------------------------------
def test_table_cache_eviction_keeps_results(G, oracle):
    """60 distinct geometries through one context and stream: the per-stream cache of coefficient tables (64 slots, dropped as a
    whole once more than 48 are taken) is evicted several times over; every result, and the first three again afterwards, is the
    oracle's."""
    img = np.random.default_rng(60).random((16, 20, 3), dtype=np.float32)
    cases = [((5 + k, 4 + k), (R.INTER_LINEAR, R.INTER_CUBIC, R.INTER_AREA)[k % 3]) for k in range(60)]
    for dsize, interp in cases + cases[:3]:
        got = G.resize(img, dsize, interp)
        assert np.array_equal(got, oracle.cv_resize(img, dsize, interp)), (dsize, interp)


# ---- 5. remap of planes ------------------------------------------------------------------------------------------------------
def edge_maps(H, W, seed):
    """Maps over the frame and 3 px beyond it, the first elements on the combinations of -1, size - 1, size - 1 + 1/64 (rounds to
    size - 1), size and -1/64 (rounds to 0) on either axis."""
    mx, my = spanning_maps(H, W, seed)
    xs = np.array([-1.0, W - 1.0, W - 1.0 + 1.0 / 64, W, -1.0 / 64], np.float32)
    ys = np.array([-1.0, H - 1.0, H - 1.0 + 1.0 / 64, H, -1.0 / 64], np.float32)
    n = min(25, H * W)
    mx.reshape(-1)[:n] = np.tile(xs, 5)[:n]
    my.reshape(-1)[:n] = np.repeat(ys, 5)[:n]
    return mx, my


def oracle_remap_planes(oracle, planes, mx, my, border):
    return np.ascontiguousarray(oracle.cv_remap_linear(np.ascontiguousarray(planes.transpose(1, 2, 0)), mx, my, border).transpose(2, 0, 1))


@pytest.mark.parametrize("size", REMAP_SIZES + [(1000, 1100)])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("border", [0.0, 0.25])
def test_remap_planes_bit_exact_vs_oracle(G, oracle, GRID, size, K, border):
    H, W = size
    assert size in REMAP_SIZES or H * W > GRID
    planes = np.random.default_rng(H + W + K).random((K, H, W), dtype=np.float32)
    mx, my = edge_maps(H, W, 11)
    got = G.remap_linear_planes(planes, mx, my, border)
    want = oracle_remap_planes(oracle, planes, mx, my, border)
    assert np.array_equal(got, want), (size, K, border, float(np.abs(got - want).max()))
    ref = R.remap64(planes.transpose(1, 2, 0), mx, my, border).transpose(2, 0, 1)
    assert float(np.abs(got - ref).max()) <= 2.0 ** -20


@pytest.mark.parametrize("size", [(37, 53), (5, 4)])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("border", [0.0, 0.25])
def test_remap_planes_nonfinite_coordinates_give_the_border(G, oracle, size, K, border):
    """NaN, +-inf and +-1e30 on either axis: cv2 converts them to INT_MIN, so the pixel takes the border value."""
    H, W = size
    planes = np.random.default_rng(H + W + K).random((K, H, W), dtype=np.float32)
    mx, my = put_nonfinite(*spanning_maps(H, W, 12))
    got = G.remap_linear_planes(planes, mx, my, border)
    n = 2 * len(NONFINITE) + 1
    assert np.array_equal(got.reshape(K, -1)[:, :n], np.full((K, n), border, np.float32)), got.reshape(K, -1)[:, :n]
    assert np.array_equal(got, oracle_remap_planes(oracle, planes, mx, my, border))


# ---- 6. Sobel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SOBEL_SIZES + [(1000, 1100)])
def test_sobel_edges_bit_exact_vs_oracle(G, oracle, GRID, size):
    assert size in SOBEL_SIZES or size[0] * size[1] > GRID
    p = np.random.default_rng(9).random(size, dtype=np.float32)
    gx, gy = G.sobel3(p)
    assert np.array_equal(gx, oracle.cv_sobel3(p, 1, 0)) and np.array_equal(gy, oracle.cv_sobel3(p, 0, 1)), size


@pytest.mark.parametrize("size", [(37, 53), (1, 7), (6, 1), (3, 2)])
def test_sobel_nonfinite_samples(G, oracle, size):
    p = np.random.default_rng(10).random(size, dtype=np.float32)
    f = p.reshape(-1)
    f[0], f[f.size // 2], f[-1] = np.inf, np.nan, -np.inf
    gx, gy = G.sobel3(p)
    assert np.array_equal(gx, oracle.cv_sobel3(p, 1, 0), equal_nan=True) and np.array_equal(gy, oracle.cv_sobel3(p, 0, 1), equal_nan=True), size


def test_planevm_sobel_batch_equals_per_frame_calls(G, ctx):
    from animal_vision_amd.planevm import DeviceBackend, PlaneRef

    H, W = 37, 53
    frames = np.random.default_rng(13).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    be = DeviceBackend(H, W, ctx=ctx, frames=2)
    try:
        gx, gy = be.sobel(be.load(PlaneRef(be.d_in, 0, 3, "u8")) * 0.25)  # channel 0 of each frame, scaled exactly
        be.flush()
        ctx.upload(frames, be.d_in)
        be.run_device()
        for f in range(2):
            wx, wy = G.sobel3(frames[f, :, :, 0].astype(np.float32) * np.float32(0.25))
            for v, want in ((gx, wx), (gy, wy)):
                ref = v.imm
                got = ctx.download(ref.buf.view(ref.offset + f * be.frame_stride(ref), 4 * H * W), (H, W), np.float32)
                assert np.array_equal(got, want), f
    finally:
        be.close()


# ---- 7. split compose --------------------------------------------------------------------------------------------------------
def split_compose(ctx, orig, mod, seam, in_place=False):
    from animal_vision_amd._lib import lib

    H, W = orig.shape[:2]
    d_o, d_m = ctx.upload(orig), ctx.upload(mod)
    d_out = d_m if in_place else ctx.malloc(orig.nbytes)  # the frame pipeline composes into the modified frame
    try:
        ctx._check(lib.avx_split_compose_u8(ctx._h, d_o.ptr, d_m.ptr, d_out.ptr, H, W, int(seam), ctx.stream))
        return ctx.download(d_out, orig.shape, np.uint8)
    finally:
        d_o.free()
        d_m.free()
        if not in_place:
            d_out.free()


@pytest.mark.parametrize("size", [(3, 1), (3, 2), (3, 3), (3, 5), (3, 64), (3, 65), (1200, 1201), (1199, 1201)])
@pytest.mark.parametrize("seam", [False, True])
def test_split_compose_vs_definition_and_oracle(ctx, oracle, GRID, size, seam):
    H, W = size
    if H > 3:
        assert H * W * 3 > 4 * GRID  # four bytes per thread: more than one pass
    if H == 1199:
        assert (H * W * 3) % 4 != 0  # the last thread's group of four is cut short
    rng = np.random.default_rng(H + W)
    a, b = rng.integers(0, 255, (H, W, 3), dtype=np.uint8), rng.integers(0, 255, (H, W, 3), dtype=np.uint8)  # no byte is 255: the seam shows
    want = R.split64(a, b, seam)
    assert np.array_equal(oracle.make_split_frame_nolabel(a, b, seam), want)
    assert np.array_equal(split_compose(ctx, a, b, seam), want), (size, seam)
    assert np.array_equal(split_compose(ctx, a, b, seam, in_place=True), want), (size, seam, "in place")


# ---- 8. binocular warp -------------------------------------------------------------------------------------------------------
WARP = dict(fov_in_deg=100.0, per_eye_half_fov_deg=105.0, overlap_deg=40.0)


@pytest.mark.parametrize("size,outs", [((1, 1), [(1, 1), (4, 3)]), ((2, 3), [(3, 2), (2, 1), (7, 5)]), ((37, 53), [(53, 37), (31, 20), (80, 61)]),
                                       ((48, 64), [(64, 48), (32, 24), (100, 75)])])
def test_binocular_warp_output_sizes_vs_oracle(G, oracle, size, outs):
    """Output (W, H) equal to, smaller than and larger than the frame's; the second frame holds only bytes <= 1 (not divided by 255)."""
    H, W = size
    frame = np.random.default_rng(H * W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for f in (frame, (frame // 128).astype(np.uint8)):
        img01 = oracle.get_normalized_image(f).astype(np.float32)
        for out_size in outs:
            got = G.animal_fov_binocular_warp_u8(f, out_size=out_size, **WARP)
            want = oracle.animal_fov_binocular_warp(img01, out_size=out_size, **WARP)
            assert got.shape == (out_size[1], out_size[0], 3) and np.array_equal(got, want), (size, out_size, int(f.max()))


def test_binocular_warp_nonfinite_coordinates_give_the_border(G, ctx, oracle, monkeypatch):
    """The warp's own remap (remap_px) under NaN, +-inf and +-1e30 column coordinates and a NaN row coordinate: that eye
    contributes the border value 0, as in the oracle driven by the same maps."""
    H, W = 37, 53
    frame = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    tables = G.binocular_warp_tables(H, W, W, H, **WARP)
    xL, xR, ymap, wL, wR = tables
    xL[:], xR[:] = np.linspace(-2.0, W + 1.0, W, dtype=np.float32), np.linspace(W + 1.0, -2.0, W, dtype=np.float32)  # both eyes see the frame
    mid = W // 2
    xL[mid - 2: mid + 3] = NONFINITE
    xR[mid + 3: mid + 8] = NONFINITE
    ymap[5] = np.nan
    wL[:], wR[:] = np.maximum(wL, np.float32(0.25)), np.maximum(wR, np.float32(0.5))  # every column shows both eyes
    grid = lambda v, axis: np.ascontiguousarray(np.broadcast_to(v[None, :] if axis else v[:, None], (H, W)))  # noqa: E731
    monkeypatch.setattr(oracle, "binocular_warp_maps", lambda *a, **k: (grid(xL, 1), grid(xR, 1), grid(ymap, 0), grid(wL, 1), grid(wR, 1)))
    want = oracle.animal_fov_binocular_warp(oracle.get_normalized_image(frame).astype(np.float32), out_size=(W, H), **WARP)
    assert not want[5].any() and want[6].any()  # the NaN row is all border
    d_in, d_out = ctx.upload(frame), ctx.malloc(4 * frame.size)
    try:
        G.binocular_warp_device(ctx, d_in, H, W, tables, H, W, d_out)
        got = ctx.download(d_out, (H, W, 3), np.float32)
    finally:
        d_in.free()
        d_out.free()
    assert np.array_equal(got, want), float(np.abs(got - want).max())


# ---- 9. panorama -------------------------------------------------------------------------------------------------------------
def test_panorama_nonfinite_source_takes_the_full_vertical_pass(G, ctx, oracle):
    """One +inf and one NaN pixel: the vertical cubic taps (0, 1, 0, 0) turn them into NaN in the rows above and below as
    well (0 * inf), so the shortcut that skips the identity vertical pass must not be taken for a caller's float data."""
    from animal_vision_amd._lib import lib

    H, W = 20, 31
    img = np.random.default_rng(20).random((H, W, 3), dtype=np.float32)
    img[4, 7, 1], img[13, 22, 2] = np.inf, np.nan
    want = oracle.panorama_warp(img, scale_x=1.12)
    assert np.isnan(want[3, :, 1]).any() and np.isnan(want[14, :, 2]).any()  # the neighbouring rows are touched: the case is live
    assert np.array_equal(G.panorama_warp(img, scale_x=1.12), want, equal_nan=True)
    new_w = max(2, int(round(W * 1.12)))
    d_in, d_out = ctx.upload(img), ctx.malloc(img.nbytes)
    try:
        ctx._check(lib.avx_panorama_warp_f32(ctx._h, d_in.ptr, H, W, new_w, d_out.ptr, ctx.stream))
        got = ctx.download(d_out, img.shape, np.float32)
    finally:
        d_in.free()
        d_out.free()
    assert np.array_equal(got, want, equal_nan=True)


def test_panorama_finite_frame_same_with_and_without_the_shortcut(ctx, oracle, monkeypatch):
    """The UV front end of a uint8 frame: fused (default), as separate launches with the horizontal-only panorama kernel
    (AVX_UV_FRONT_SPLIT), and with the full two-pass cubic forced (AVX_PANO_FULL): one linear frame, the oracle's warp of the
    decoded frame."""
    from animal_vision_amd._lib import lib

    H, W = 20, 31
    frame = np.random.default_rng(21).integers(0, 256, (H, W, 3), dtype=np.uint8)
    new_w = max(2, int(round(W * 1.12)))
    d_in, d_lin, d_base = ctx.upload(frame), ctx.malloc(4 * frame.size), ctx.malloc(frame.size)

    def front(nw):
        ctx._check(lib.avx_uv_front_u8(ctx._h, d_in.ptr, H, W, nw, d_lin.ptr, d_base.ptr, ctx.stream))
        return ctx.download(d_lin, frame.shape, np.float32), ctx.download(d_base, frame.shape, np.uint8)

    try:
        monkeypatch.delenv("AVX_UV_FRONT_SPLIT", raising=False)
        monkeypatch.delenv("AVX_PANO_FULL", raising=False)
        decoded, _ = front(W)
        fused = front(new_w)
        monkeypatch.setenv("AVX_UV_FRONT_SPLIT", "1")
        short = front(new_w)
        monkeypatch.setenv("AVX_PANO_FULL", "1")
        full = front(new_w)
    finally:
        for b in (d_in, d_lin, d_base):
            b.free()
    want = oracle.panorama_warp(decoded, scale_x=1.12)
    for name, (lin, base) in (("fused", fused), ("shortcut", short), ("full", full)):
        assert np.array_equal(lin, want), name
        assert np.array_equal(base, full[1]), name
