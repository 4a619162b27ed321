"""GPU: the species wall.

  * avx_wall_compose_u8 (csrc/wall.hip: a resident layout, one launch per batch) against avx_gallery_compose_u8 called per frame
    on the same device, byte for byte on the gallery's canvas and bg outside it; one case per resize mode anchored to the CPU
    restatement of build_labeled_grid (oracle_grid of tests/test_gallery_gpu.py).
  * its refusals, each followed by a good call on the same context; avx_memcpy_d2d against a download.
  * WallStreamOp through FramePipeline and the `wall` command against build_labeled_grid over the species' visualize() outputs."""
import ctypes
import itertools

import numpy as np
import pytest

import _yuv_ref as R
from test_gallery_gpu import LONGEST, oracle_grid

pytestmark = pytest.mark.gpu

NAMES = [LONGEST, "Dog", "Cat", "HoneyBee", "ReinDeer", "Fox", "Pig"]  # tile 0's label is wider than any tile here: clipped
BG = (20, 30, 40)
MODES = {"copy": 0, "area_fast": 1, "area": 2, "linear": 3}


@pytest.fixture(scope="module")
def ctx():
    from animal_vision_amd.runtime import get_context

    return get_context()


def _noise(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


class _Wall:
    """n tiles of n_frames H x W frames on the device (frame stride above a frame, odd tile bases: no source pointer is aligned),
    a wall layout over them, and the canvases of both entry points."""

    def __init__(self, ctx, H, W, tile_height, n, n_frames, *, labels=True, pad=8, cols=None, seed=0):
        from animal_vision_amd._lib import lib
        from animal_vision_amd.gallery_grid import STRIP_H, GridLayout

        self.ctx, self.H, self.W, self.n, self.F, self.pad = ctx, H, W, n, n_frames, pad
        self.names = NAMES[:n]
        grid = GridLayout(self.names, [(H, W)] * n, tile_height, pad)
        self.h, self.w = grid.sizes[0]
        self.cols = grid.cols if cols is None else cols
        self.strip = STRIP_H if labels else 0
        self.segs = np.ascontiguousarray(grid.segments if labels else np.zeros((0, 6), np.float32), np.float32)
        self.seg_off = list(grid.seg_offsets) if labels else [0] * n
        self.seg_cnt = list(grid.seg_counts) if labels else [0] * n
        rows = -(-n // self.cols)
        self.grid_hw = (rows * (self.h + self.strip + pad) + pad, self.cols * (self.w + pad) + pad)
        self.frames = _noise(seed, n, n_frames, H, W, 3)
        self.stride = H * W * 3 + 37                      # bytes from frame to frame of one tile
        tile_bytes = (n_frames * self.stride + 64) | 1    # odd: consecutive tiles start at every alignment
        host = np.zeros(n * tile_bytes + 16, np.uint8)
        self.offs = [1 + i * tile_bytes for i in range(n)]
        for i in range(n):
            for f in range(n_frames):
                o = self.offs[i] + f * self.stride
                host[o:o + H * W * 3] = self.frames[i, f].reshape(-1)
        self.d_src = ctx.upload(host)
        handle = ctypes.c_void_p()
        ctx._check(lib.avx_wall_layout_create(ctx._h, H, W, self.h, self.w, n, (ctypes.c_int * n)(*self.seg_off), (ctypes.c_int * n)(*self.seg_cnt),
                                              self.segs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(self.segs), self.strip, pad, self.cols,
                                              (ctypes.c_int * 3)(*BG), ctypes.byref(handle)))
        self.layout = handle.value
        hc, wc = ctypes.c_int(), ctypes.c_int()
        assert lib.avx_wall_canvas_size(self.layout, ctypes.byref(hc), ctypes.byref(wc)) == 0
        self.Hc, self.Wc = hc.value, wc.value
        assert (self.Hc, self.Wc) == tuple(v + (v & 1) for v in self.grid_hw)

    def info(self):
        from animal_vision_amd._lib import lib

        mode, staged, piece, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert lib.avx_wall_layout_info(self.layout, ctypes.byref(mode), ctypes.byref(staged), ctypes.byref(piece), ctypes.byref(lds)) == 0
        return mode.value, staged.value, piece.value, lds.value

    def src_ptrs(self):
        return (ctypes.c_void_p * self.n)(*(self.d_src.ptr + o for o in self.offs))

    def wall(self, n_frames=None):
        """The canvases of one avx_wall_compose_u8 call: canvas stride above a frame, the first canvas at an odd address."""
        from animal_vision_amd._lib import lib

        F = self.F if n_frames is None else n_frames
        cbytes = self.Hc * self.Wc * 3
        cstride = cbytes + 53
        d = self.ctx.malloc(3 + self.F * cstride)
        self.ctx.memset(d, 0xAB)
        self.ctx._check(lib.avx_wall_compose_u8(self.ctx._h, self.layout, self.src_ptrs(), self.stride, F, d.ptr + 3, cstride, self.ctx._s(None)))
        raw = self.ctx.download(d, (3 + self.F * cstride,), np.uint8)
        d.free()
        assert (raw[:3] == 0xAB).all(), "bytes in front of the first canvas were written"
        out = []
        for f in range(self.F):
            o = 3 + f * cstride
            if f < F:
                out.append(raw[o:o + cbytes].reshape(self.Hc, self.Wc, 3))
                assert (raw[o + cbytes:o + cstride] == 0xAB).all(), f"bytes behind canvas {f} were written"
            else:
                assert (raw[o:o + cstride] == 0xAB).all(), f"canvas {f} lies beyond n_frames and was written"
        return out

    def gallery(self, f):
        """Frame f through avx_gallery_compose_u8 on the gallery's own canvas."""
        from animal_vision_amd._lib import GalleryTile, lib

        Hg, Wg = self.grid_hw
        d = self.ctx.malloc(Hg * Wg * 3)
        desc = (GalleryTile * self.n)(*(GalleryTile(self.d_src.ptr + self.offs[i] + f * self.stride, 2, self.H, self.W, self.h, self.w, self.seg_off[i],
                                                    self.seg_cnt[i]) for i in range(self.n)))
        self.ctx._check(lib.avx_gallery_compose_u8(self.ctx._h, desc, self.n, self.segs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(self.segs),
                                                   self.strip, self.pad, self.cols, (ctypes.c_int * 3)(*BG), d.ptr, Hg, Wg, self.ctx._s(None)))
        out = self.ctx.download(d, (Hg, Wg, 3), np.uint8)
        d.free()
        return out

    def check(self, n_frames=None, what=""):
        got = self.wall(n_frames)
        Hg, Wg = self.grid_hw
        for f, canvas in enumerate(got):
            want = self.gallery(f)
            bad = np.argwhere((canvas[:Hg, :Wg] != want).any(-1))
            assert bad.size == 0, f"{what} frame {f}: {len(bad)} pixels differ from avx_gallery_compose_u8, first at {bad[:3].tolist()}"
            assert (canvas[Hg:] == np.asarray(BG, np.uint8)).all() and (canvas[:, Wg:] == np.asarray(BG, np.uint8)).all(), f"{what} frame {f}: not bg outside the grid"
        return got

    def close(self):
        from animal_vision_amd._lib import lib

        self.ctx._check(lib.avx_wall_layout_destroy(self.ctx._h, self.layout))
        self.d_src.free()


# (source H, W, tile height, mode): the smallest shapes that reach every branch -- the integer ratio 4, two general ratios of odd
# sizes, no resize, enlarging; then a 2 x 2 ratio (cv2's 8-bit rounding) and sources one pixel wider than a 16-byte vector's 16
# pixels / than the staged rows' multiple of 16 pixels, whose row segments end in a tail of single bytes
CASES = [(64, 96, 16, "area_fast"), (36, 50, 16, "area"), (37, 51, 16, "area"), (16, 24, 16, "copy"), (12, 20, 16, "linear"),
         (32, 34, 16, "area_fast"), (16, 17, 16, "copy"), (64, 68, 16, "area_fast")]


@pytest.mark.parametrize("H, W, th, mode", CASES)
def test_wall_equals_the_gallery_per_frame(ctx, H, W, th, mode):
    """n_tiles 1, 2, 5, 7 (a ragged last row; 5 and 7 leave empty cells) x n_frames 1, 3, 16, labels and pad alternating so that every
    (labels, pad) pair meets every mode; frame strides above a frame on both sides, unaligned sources and canvases."""
    seen = set()
    for idx, (n, F) in enumerate(itertools.product((1, 2, 5, 7), (1, 3, 16))):
        labels, pad = idx % 2 == 0, 8 if (idx // 2) % 2 == 0 else 0
        seen.add((labels, pad))
        w = _Wall(ctx, H, W, th, n, F, labels=labels, pad=pad, seed=idx)
        try:
            m, staged, _, _ = w.info()
            assert m == MODES[mode] and staged == 1
            odd = (w.grid_hw[0] & 1, w.grid_hw[1] & 1)
            w.check(what=f"n={n} F={F} labels={labels} pad={pad} odd={odd}")
        finally:
            w.close()
    assert len(seen) == 4


def test_even_rounding_adds_a_row_and_a_column(ctx):
    """Three 37 x 51 tiles at pad 7 without labels: the gallery's canvas is 53 x 65, the wall's has one more bg row and column."""
    w = _Wall(ctx, 37, 51, 16, 3, 2, labels=False, pad=7)
    try:
        assert w.grid_hw[0] % 2 == 1 and w.grid_hw[1] % 2 == 1 and (w.Hc, w.Wc) == (w.grid_hw[0] + 1, w.grid_hw[1] + 1)
        w.check()
    finally:
        w.close()


@pytest.mark.parametrize("H, W, th, mode", [(16, 300, 16, "copy"), (32, 600, 16, "area_fast"), (36, 650, 16, "area"), (12, 220, 16, "linear")])
def test_tiles_wider_than_a_piece(ctx, H, W, th, mode):
    """Tiles of about 300 pixels: a column is more than one workgroup's piece of 256 pixels."""
    w = _Wall(ctx, H, W, th, 3, 2, labels=True, pad=8, seed=5)
    try:
        m, staged, piece, _ = w.info()
        assert m == MODES[mode] and staged == 1 and piece < w.w
        w.check()
    finally:
        w.close()


@pytest.mark.parametrize("H, W, mode", [(512, 768, "area_fast"), (500, 770, "area")])
def test_bands_too_large_for_lds_read_the_source(ctx, H, W, mode):
    """A 32-fold reduction: the band of source rows under one row of samples is above the workgroup's LDS budget, the layout says
    it is not staged, and the canvas is the same."""
    w = _Wall(ctx, H, W, 16, 2, 2, labels=True, pad=8, seed=9)
    try:
        m, staged, _, _ = w.info()
        assert m == MODES[mode] and staged == 0
        w.check()
    finally:
        w.close()


def test_a_cols_argument_that_leaves_empty_cells(ctx):
    w = _Wall(ctx, 36, 50, 16, 2, 1, cols=3)
    try:
        w.check()
    finally:
        w.close()


def test_fewer_frames_than_the_buffers_hold(ctx):
    w = _Wall(ctx, 36, 50, 16, 2, 3)
    try:
        w.check(n_frames=2)   # the third canvas stays untouched (checked in wall())
        w.check(n_frames=0)   # AVX_OK, nothing launched
    finally:
        w.close()


@pytest.mark.parametrize("H, W, th", [(64, 96, 16), (37, 51, 16), (16, 24, 16), (12, 20, 16)])
def test_wall_equals_the_cpu_restatement(ctx, H, W, th):
    """One case per mode against build_labeled_grid restated on the oracle (cv_resize INTER_AREA, draw_label_pixels, NumPy placement)."""
    w = _Wall(ctx, H, W, th, 5, 2, labels=True, pad=8, seed=21)
    try:
        got = w.wall()
        Hg, Wg = w.grid_hw
        for f in range(2):
            want = oracle_grid([(w.names[i], w.frames[i, f]) for i in range(5)], tile_height=th, pad=8, bg=BG)
            assert want.shape == (Hg, Wg, 3)
            bad = np.argwhere((got[f][:Hg, :Wg] != want).any(-1))
            assert bad.size == 0, f"frame {f}: {len(bad)} pixels differ from the oracle, first at {bad[:3].tolist()}"
    finally:
        w.close()


def test_refusals_leave_the_context_usable(ctx):
    from animal_vision_amd._lib import AVX_ERR_INVALID, AVX_EW_MAX_FRAMES, AvxError, lib
    from animal_vision_amd.runtime import Context

    w = _Wall(ctx, 36, 50, 16, 2, 2)
    other = Context(ctx.device)
    try:
        cbytes, sbytes = w.Hc * w.Wc * 3, w.H * w.W * 3
        canvas = ctx.malloc(AVX_EW_MAX_FRAMES * cbytes + 64)
        good = dict(h=ctx._h, layout=w.layout, src=w.src_ptrs(), sstride=w.stride, n=2, canvas=canvas.ptr, cstride=cbytes)

        def call(**kw):
            a = dict(good, **kw)
            return lib.avx_wall_compose_u8(a["h"], a["layout"], a["src"], a["sstride"], a["n"], a["canvas"], a["cstride"], ctx._s(None))

        def ptrs(*p):
            return (ctypes.c_void_p * 2)(*p)

        s0, s1 = w.d_src.ptr + w.offs[0], w.d_src.ptr + w.offs[1]
        bad = {
            "layout NULL": dict(layout=None),
            "src NULL": dict(src=None),
            "canvas NULL": dict(canvas=None),
            "a source NULL": dict(src=ptrs(s0, None)),
            "a source equal to the canvas": dict(src=ptrs(s0, canvas.ptr)),
            "a source inside the canvas": dict(src=ptrs(canvas.ptr + cbytes + 5, s1)),
            "the canvas inside a source's frames": dict(canvas=s1 + w.stride - 4),
            "source stride below a frame": dict(sstride=sbytes - 1),
            "canvas stride below a frame": dict(cstride=cbytes - 1),
            "batch above the cap": dict(n=AVX_EW_MAX_FRAMES + 1),
            "negative batch": dict(n=-1),
            "a layout of another context": dict(h=other._h),
        }
        for what, kw in bad.items():
            rc = call(**kw)
            assert rc == AVX_ERR_INVALID, what
            c = other if "h" in kw else ctx
            assert lib.avx_last_error(c._h).decode().startswith("avx_wall_compose_u8"), what
            with pytest.raises(AvxError, match="avx_wall_compose_u8"):
                c._check(rc)
            assert call() == 0, f"a good call after: {what}"
        ctx.sync()
        got = ctx.download(canvas, (2, w.Hc, w.Wc, 3), np.uint8)
        Hg, Wg = w.grid_hw
        for f in range(2):
            assert np.array_equal(got[f][:Hg, :Wg], w.gallery(f))
        canvas.free()
        # the layout's own refusals
        handle = ctypes.c_void_p()
        bg = (ctypes.c_int * 3)(*BG)
        for args in [(0, 50, 16, 22, 2), (36, 50, 16, 22, 0), (36, 50, 16, 22, 65)]:
            Hs, Ws, h, wd, n = args
            rc = lib.avx_wall_layout_create(ctx._h, Hs, Ws, h, wd, n, None, None, None, 0, 0, 8, 1, bg, ctypes.byref(handle))
            assert rc == AVX_ERR_INVALID and handle.value is None and lib.avx_last_error(ctx._h).decode().startswith("avx_wall_layout_create"), args
        assert lib.avx_wall_layout_destroy(other._h, w.layout) == AVX_ERR_INVALID  # not the other context's to destroy
        w.check()
    finally:
        w.close()
        other.close()


def test_memcpy_d2d_against_a_download(ctx):
    from animal_vision_amd._lib import AVX_ERR_INVALID, lib

    a = _noise(3, 100_003)
    src, dst = ctx.upload(a), ctx.malloc(a.size + 16)
    ctx.memset(dst, 0x5A)
    s = ctx.stream_create()
    ctx._check(lib.avx_memcpy_d2d(ctx._h, dst.ptr + 7, src.ptr + 2, a.size - 2, s))
    got = ctx.download(dst, (a.size + 16,), np.uint8, stream=s)  # ordered behind the copy on its stream
    assert (got[:7] == 0x5A).all() and np.array_equal(got[7:7 + a.size - 2], a[2:]) and (got[7 + a.size - 2:] == 0x5A).all()
    assert lib.avx_memcpy_d2d(ctx._h, None, src.ptr, 4, s) == AVX_ERR_INVALID
    assert lib.avx_last_error(ctx._h).decode().startswith("avx_memcpy_d2d")
    ctx._check(lib.avx_memcpy_d2d(ctx._h, dst.ptr, src.ptr, 0, s))
    ctx.sync(s)
    ctx.stream_destroy(s)
    src.free()
    dst.free()


# ---------------------------------------------------------------- the operator and the pipeline ------------------------------------
WALL = ["Dog", "Cat", "HoneyBee", "ReinDeer"]
TILE_H = 32


def _members():
    from animal_vision_amd.gallery import species_class

    return [(n, species_class(n)()) for n in WALL]


def _even(img, bg=(20, 20, 20)):
    H, W = img.shape[:2]
    out = np.empty((H + (H & 1), W + (W & 1), 3), np.uint8)
    out[...] = np.asarray(bg, np.uint8)
    out[:H, :W] = img
    return out


_species = {}


def _expected(frames, labels=True):
    """build_labeled_grid over [Original] + the species' visualize() outputs of every frame, padded to even."""
    from animal_vision_amd.gallery import _output_of, species_class
    from animal_vision_amd.gallery_grid import build_labeled_grid

    for n in WALL:
        if n not in _species:
            _species[n] = species_class(n)()
    out = []
    for f in frames:
        tiles = [("Original", f)] + [(n, _output_of(_species[n].visualize(f))) for n in WALL]
        assert labels
        out.append(_even(build_labeled_grid(tiles, tile_height=TILE_H, pad=8)))
    return out


def _frames(H, W, n, seed=40):
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    return [(structured_frame if i % 2 else noise_frame)(seed + i, H, W) for i in range(n)]


@pytest.fixture(scope="module")
def streams():
    """Per frame size: 6 frames and their expected sheets, computed once."""
    out = {}
    for H, W in [(48, 64), (54, 96)]:
        frames = _frames(H, W, 6)
        out[(H, W)] = (frames, _expected(frames))
    return out


def _through_pipeline(op, frames, H, W, **kw):
    from animal_vision_amd.pipeline import FramePipeline

    pipe = FramePipeline(op, H, W, **kw)
    got = {}
    try:
        st = pipe.run(iter(enumerate(frames)), lambda i, o: got.__setitem__(i, o.copy()))
    finally:
        pipe.close()
    assert st.frames == len(frames) and sorted(got) == list(range(len(frames)))
    return [got[i] for i in range(len(frames))], st, (pipe.out_H, pipe.out_W)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("hw, batch, depth", [((48, 64), 1, 2), ((48, 64), 4, 3), ((54, 96), 4, 2), ((54, 96), 1, 3)])
def test_wall_stream_equals_the_grid_of_visualize(ctx, streams, hw, batch, depth):
    """6 frames: at batch 4 a full slot and a partial one.  54 x 96 lays out on 168 x 203: the even rounding adds a column."""
    from animal_vision_amd.wall import WallStreamOp

    H, W = hw
    frames, want = streams[hw]
    op = WallStreamOp(_members(), H, W, tile_height=TILE_H, depth=depth, batch=batch)
    try:
        assert op.max_batch >= batch and op.out_shape(H, W) == want[0].shape[:2]
        got, st, out_hw = _through_pipeline(op, frames, H, W, depth=depth, batch=batch)
    finally:
        op.close()
    assert out_hw == want[0].shape[:2] and st.pixels == len(frames) * H * W  # the pixels the op saw
    for k in range(len(frames)):
        _same(got[k], want[k], (hw, batch, depth, k))


def test_a_plane_program_species_through_the_wall_equals_its_own_stream(ctx, streams):
    """ReinDeer alone, without labels or the original, at tile height = frame height: the sheet is its stream's frame inside the pad."""
    from animal_vision_amd.gallery import species_class
    from animal_vision_amd.video import stream_op
    from animal_vision_amd.wall import WallStreamOp

    H, W = 48, 64
    frames = streams[(H, W)][0]
    own = stream_op(species_class("ReinDeer")(), H, W, 2, 4)
    try:
        want, _, _ = _through_pipeline(own, frames, H, W, depth=2, batch=4)
    finally:
        own.close()
    op = WallStreamOp([("ReinDeer", species_class("ReinDeer")())], H, W, tile_height=H, pad=8, labels=False, original=False, depth=2, batch=4)
    try:
        assert op.out_shape(H, W) == (H + 16, W + 16)
        got, _, _ = _through_pipeline(op, frames, H, W, depth=2, batch=4)
    finally:
        op.close()
    for k in range(len(frames)):
        _same(got[k][8:8 + H, 8:8 + W], want[k], k)
        border = got[k].copy()
        border[8:8 + H, 8:8 + W] = 20
        assert (border == 20).all()


@pytest.mark.parametrize("io_format", ["i420", "yuv"])
def test_wall_stream_of_payloads(ctx, io_format):
    """I420 and nv12 payloads in, the encode of the sheet out."""
    from animal_vision_amd import yuv
    from animal_vision_amd.wall import WallStreamOp

    H, W = 48, 64
    rgb = np.stack(_frames(H, W, 5, seed=60))
    if io_format == "i420":
        payloads, kw = R.encode(rgb), {}
        decoded = R.decode(payloads, H, W)
    else:
        payloads, kw = yuv.rgb_to_yuv(rgb, pix_fmt="nv12"), dict(pix_fmt="nv12")
        decoded = yuv.yuv_to_rgb(payloads, H, W, pix_fmt="nv12")
    want = _expected(list(decoded))
    op = WallStreamOp(_members(), H, W, tile_height=TILE_H, depth=2, batch=2)
    try:
        got, _, out_hw = _through_pipeline(op, list(payloads), H, W, depth=2, batch=2, io_format=io_format, **kw)
    finally:
        op.close()
    for k in range(5):
        enc = R.encode(want[k][None])[0] if io_format == "i420" else yuv.rgb_to_yuv(want[k], pix_fmt="nv12")
        assert got[k].shape == (yuv.frame_size("nv12", *out_hw),)
        _same(got[k], enc.reshape(-1), (io_format, k))


def test_members_of_the_per_frame_loop_are_refused_before_device_work(ctx):
    from animal_vision_amd.animals import HoneyBee, MantisShrimp
    from animal_vision_amd.wall import WallStreamOp

    with pytest.raises(ValueError, match="Mantis"):
        WallStreamOp([("Dog", _members()[0][1]), ("Mantis Shrimp", MantisShrimp())], 48, 64)
    with pytest.raises(ValueError, match="bee"):
        WallStreamOp([("bee", HoneyBee(hsi_downsample=True, hsi_scale=0.5))], 48, 64)


# ---------------------------------------------------------------- the command ------------------------------------------------------
def _read_y4m(path):
    from animal_vision_amd.renderers.y4m import Y4MReader

    rd = Y4MReader(path)
    out = []
    while (f := rd.read()) is not None:
        out.append(f)
    hdr = rd.header
    rd.close()
    return hdr, out


def test_command_y4m_to_y4m(tmp_path, capsys):
    from animal_vision_amd.wall import main

    H, W = 54, 96
    rgb = np.stack(_frames(H, W, 5, seed=80))
    payloads = R.encode(rgb)
    src, dst, dst4 = str(tmp_path / "in.y4m"), str(tmp_path / "wall.y4m"), str(tmp_path / "wall4.y4m")
    with open(src, "wb") as f:
        f.write(R.y4m_bytes(list(payloads), H, W))
    argv = ["--species", ",".join(WALL), "--tile-height", str(TILE_H)]
    assert main([src, dst] + argv) == 0
    assert "5 frames" in capsys.readouterr().err
    assert main([src, dst4] + argv + ["--batch", "4", "--depth", "2"]) == 0
    assert open(dst, "rb").read() == open(dst4, "rb").read()
    want = _expected(list(R.decode(payloads, H, W)))
    hdr, frames = _read_y4m(dst)
    assert (hdr.height, hdr.width) == want[0].shape[:2] == (168, 204) and len(frames) == 5  # the sheet's size, not the input's
    for k in range(5):
        _same(frames[k], R.encode(want[k][None])[0], k)


def test_command_rgb_sinks(tmp_path, capsys):
    """synthetic: in, .npy and a PNG directory out: RGB frames of the sheet's size."""
    from PIL import Image

    from animal_vision_amd.renderers import VideoRenderer
    from animal_vision_amd.wall import main

    H, W = 48, 64
    vr = VideoRenderer(read_path=f"synthetic:{W}x{H}:3")
    vr.open()
    frames = [vr.get_image() for _ in range(3)]
    vr.close()
    want = _expected(frames)
    npy, pngs = str(tmp_path / "wall.npy"), str(tmp_path / "pngs")
    argv = ["--species", ",".join(WALL), "--tile-height", str(TILE_H)]
    assert main([f"synthetic:{W}x{H}:3", npy] + argv) == 0
    assert main([f"synthetic:{W}x{H}:3", pngs] + argv) == 0
    got = np.load(npy)
    assert got.shape == (3,) + want[0].shape
    for k in range(3):
        _same(got[k], want[k], ("npy", k))
        _same(np.asarray(Image.open(f"{pngs}/frame_{k:06d}.png").convert("RGB")), want[k], ("png", k))


def test_command_raw_nv12_scaled(tmp_path, capsys):
    from animal_vision_amd import yuv
    from animal_vision_amd.wall import main

    H, W, Hd, Wd, fmt = 96, 128, 48, 64, "nv12"
    payloads = yuv.rgb_to_yuv(np.stack(_frames(H, W, 3, seed=90)), pix_fmt=fmt)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "wall.yuv")
    payloads.tofile(src)
    assert main([src, dst, "--species", ",".join(WALL), "--tile-height", str(TILE_H), "--pix-fmt", fmt, "--size", f"{W}x{H}", "--scale", f"{Wd}x{Hd}",
                 "--batch", "2"]) == 0
    assert "3 frames" in capsys.readouterr().err
    want = _expected(list(yuv.yuv_to_rgb_scaled(payloads, H, W, Hd, Wd, pix_fmt=fmt)))
    got = np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(3, -1)
    assert got.shape[1] == yuv.frame_size(fmt, *want[0].shape[:2])  # the raw frame size is the sheet's
    for k in range(3):
        _same(got[k], yuv.rgb_to_yuv(want[k], pix_fmt=fmt).reshape(-1), k)


def test_command_hdr_pq(tmp_path, capsys):
    from animal_vision_amd import yuv
    from animal_vision_amd.wall import main

    H, W, fmt = 48, 64, "p010le"
    payloads = yuv.rgb_to_yuv(np.stack(_frames(H, W, 2, seed=95)), pix_fmt=fmt)  # any 10-bit payload will do as PQ code values
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "wall.yuv")
    payloads.tofile(src)
    assert main([src, dst, "--species", ",".join(WALL), "--tile-height", str(TILE_H), "--pix-fmt", fmt, "--size", f"{W}x{H}", "--transfer", "pq"]) == 0
    want = _expected(list(yuv.yuv_hdr_to_rgb(payloads, H, W, pix_fmt=fmt, transfer="pq")))
    got = np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(2, -1)
    assert got.shape[1] == yuv.frame_size(fmt, *want[0].shape[:2])
    for k in range(2):
        _same(got[k], yuv.rgb_to_yuv(want[k], pix_fmt=fmt, matrix="bt709").reshape(-1), k)


def test_command_category_drops_the_per_frame_species(tmp_path, capsys):
    from animal_vision_amd.gallery import CATEGORIES
    from animal_vision_amd.wall import main

    npy = str(tmp_path / "uu.npy")
    assert main(["synthetic:64x48:2", npy, "--category", "Unique-UV", "--tile-height", "24", "--no-original"]) == 0
    err = capsys.readouterr().err
    assert "dropped Mantis Shrimp" in err and f"{len(CATEGORIES['Unique-UV']) - 1} species: 2 frames" in err
    assert np.load(npy).shape[0] == 2
