"""The species wall: every frame of a video through several species at once, the outputs laid out as the `gallery` command's
labelled grid -- one frame decoded and uploaded, one composed sheet of tile-height images sent back:

    python -m animal_vision_amd.wall in.y4m wall.y4m --species Dog,Cat,HoneyBee,ReinDeer
    ffmpeg -i in.mkv -f rawvideo -pix_fmt nv12 - | python -m animal_vision_amd.wall - wall.yuv --category Non-UV --pix-fmt nv12 --size 3840x2160

`--species` takes display names of gallery.py's registry separated by commas; `--category` takes a whole category of it.  The
first tile is the input frame, labelled "Original" (`--no-original`: none); `--tile-height`, `--pad` and `--no-labels` shape the
sheet as gallery_grid.build_labeled_grid shapes it.  INPUT, OUTPUT and the I/O options (`--depth`, `--batch`, `--matrix`, `--range`,
`--pix-fmt`, `--size`, `--scale`, `--out-pix-fmt`, `--transfer` and its companions, `--out-matrix`) are the `video` command's.  The
output has the sheet's size (both dimensions even), not the input's.

Only species with a stream operator (video.has_stream_op) can stand on a wall: the species of the per-frame loop (Mantis Shrimp,
RatUV) are an error with `--species`, and dropped with a line on stderr from a `--category`.

WallStreamOp is the operator behind it (pipeline.FramePipeline's protocol): per pipeline slot it runs its members one after the
other on the slot's stream, all reading the slot's one input, and composes their outputs with one avx_wall_compose_u8 launch
(csrc/wall.hip) whose layout -- resize tables, label segments, grid -- went to the device once, when the op was built."""
from __future__ import annotations

import argparse
import ctypes
import sys
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .gallery import CATEGORIES, _CLASS_NAMES, species_class
from .gallery_grid import STRIP_H, GridLayout, check_tiles

ORIGINAL_LABEL = "Original"


class WallLayout:
    """A wall's sheet without its pixels (host arithmetic only): n tiles of H x W sources under `labels`, laid out by
    gallery_grid.GridLayout.  with_labels=False: no strip under the tiles and no segments."""

    def __init__(self, labels: Sequence[str], H: int, W: int, tile_height: int = 256, pad: int = 8, with_labels: bool = True):
        if not labels:
            raise ValueError("a wall needs at least one tile")
        grid = GridLayout(list(labels), [(int(H), int(W))] * len(labels), int(tile_height), int(pad))
        self.labels, self.n, self.H, self.W, self.pad = list(labels), len(labels), int(H), int(W), int(pad)
        self.h, self.w = grid.sizes[0]
        self.cols, self.rows = grid.cols, grid.rows
        self.strip_h = STRIP_H if with_labels else 0
        self.cell_h, self.cell_w = self.h + self.strip_h + self.pad, grid.cell_w
        self.grid_shape = (self.rows * self.cell_h + self.pad, self.cols * self.cell_w + self.pad)  # the gallery's canvas
        self.canvas_shape = tuple(v + (v & 1) for v in self.grid_shape)                               # ... rounded up to even
        if with_labels:
            self.segments, self.seg_offsets, self.seg_counts = grid.segments, list(grid.seg_offsets), list(grid.seg_counts)
        else:
            self.segments, self.seg_offsets, self.seg_counts = np.zeros((0, 6), np.float32), [0] * self.n, [0] * self.n


def per_frame_names(names: Sequence[str]) -> List[str]:
    """Those of the display names whose species run visualize() per frame (no stream operator: they cannot stand on a wall)."""
    from .video import has_stream_op

    return [n for n in names if not has_stream_op(species_class(n)())]


class WallStreamOp:
    """Several species on every frame, composed into one labelled grid (pipeline.FramePipeline's protocol, with out_shape).

    members: (label, animal) pairs; original=True puts the input frame first, labelled "Original".  Every member must have a
    stream operator (video.has_stream_op; video.stream_op builds it with this wall's depth and batch): a species of the
    per-frame loop is a ValueError naming it, raised before any device work.  Members that take any device pointers (DichromatOp,
    HoneybeeOp) read the slot's input and write a buffer of this op; members that own their slot buffers (CatStreamOp,
    SpeciesStreamOp, MstHoneybeeStreamOp) get the input copied into theirs on the slot's stream.  The buffers are plain
    allocations of the op, which outlive the slot streams."""

    def __init__(self, members: Sequence[Tuple[str, object]], H: int, W: int, *, tile_height: int = 256, pad: int = 8,
                 bg: Tuple[int, int, int] = (20, 20, 20), labels: bool = True, original: bool = True, depth: int = 3, batch: int = 1, ctx=None):
        from .video import has_stream_op

        members = list(members)
        check_tiles([], tile_height, pad, bg)
        if not members and not original:
            raise ValueError("a wall needs at least one tile")
        for label, animal in members:
            if not isinstance(label, str):
                raise TypeError(f"a member's label must be a str (got {type(label).__name__})")
            if not has_stream_op(animal):
                raise ValueError(f"{label}: {type(animal).__name__} runs visualize() per frame and has no stream operator: it cannot stand on a wall")
        if depth < 1 or batch < 1:
            raise ValueError(f"depth and batch must be at least 1 (got {depth} and {batch})")
        self.H, self.W, self.depth, self.batch = int(H), int(W), int(depth), int(batch)
        self.original, self.bg = bool(original), tuple(int(v) for v in bg)
        self.layout = WallLayout(([ORIGINAL_LABEL] if original else []) + [label for label, _ in members], self.H, self.W, tile_height, pad, labels)
        self._layout_h = None
        self._ops, self._outs, self._bufs, self._src = [], [], [], []

        from ._lib import AVX_EW_MAX_FRAMES, lib
        from .runtime import get_context
        from .video import stream_op

        if self.layout.n > lib.avx_wall_max_tiles():
            raise ValueError(f"a wall takes at most {lib.avx_wall_max_tiles()} tiles (got {self.layout.n})")
        self.ctx = ctx or get_context()
        try:
            for label, animal in members:
                op = stream_op(animal, self.H, self.W, self.depth, self.batch)
                self._ops.append((label, op))
                if getattr(op, "ctx", None) is None:
                    op.ctx = self.ctx
            self.max_batch = min([AVX_EW_MAX_FRAMES] + [getattr(op, "max_batch", 1) for _, op in self._ops])
            if self.batch > self.max_batch:
                raise ValueError(f"batch={self.batch}: the wall's members take at most {self.max_batch} frame(s) per call")
            lay = self.layout
            seg = np.ascontiguousarray(lay.segments, np.float32)
            handle = ctypes.c_void_p()
            self.ctx._check(lib.avx_wall_layout_create(
                self.ctx._h, self.H, self.W, lay.h, lay.w, lay.n, (ctypes.c_int * lay.n)(*lay.seg_offsets), (ctypes.c_int * lay.n)(*lay.seg_counts),
                seg.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(seg), lay.strip_h, lay.pad, lay.cols, (ctypes.c_int * 3)(*self.bg),
                ctypes.byref(handle)))
            self._layout_h = handle.value
            hc, wc = ctypes.c_int(), ctypes.c_int()
            self.ctx._check(lib.avx_wall_canvas_size(self._layout_h, ctypes.byref(hc), ctypes.byref(wc)))
            if (hc.value, wc.value) != lay.canvas_shape:
                raise RuntimeError(f"the library lays the wall out on {hc.value} x {wc.value}, the host on {lay.canvas_shape[0]} x {lay.canvas_shape[1]}")
            in_bytes, out_bytes = self.batch * self.H * self.W * 3, self.batch * lay.canvas_shape[0] * lay.canvas_shape[1] * 3
            for k in range(self.depth):
                self._bufs.append((self.ctx.malloc(in_bytes), self.ctx.malloc(out_bytes)))
                outs, src = [], ([self._bufs[k][0].ptr] if self.original else [])
                for _, op in self._ops:
                    lend = getattr(op, "slot_buffers", None)
                    outs.append(None if lend is not None else self.ctx.malloc(in_bytes))
                    src.append(lend(k)[1].ptr if lend is not None else outs[-1].ptr)
                self._outs.append(outs)
                self._src.append((ctypes.c_void_p * lay.n)(*src))  # a slot's sources never move: the pointer array is built once
        except Exception:
            self.close()
            raise
        self._by_in = {d_in.ptr: k for k, (d_in, _) in enumerate(self._bufs)}

    def out_shape(self, H: int, W: int) -> Tuple[int, int]:
        """(Hc, Wc) of the sheet this op writes for H x W frames (the size it was built for)."""
        if (int(H), int(W)) != (self.H, self.W):
            raise ValueError(f"this wall was built for {self.H} x {self.W} frames (got {H} x {W})")
        return self.layout.canvas_shape

    def slot_buffers(self, k: int):
        return self._bufs[k]

    def run_device(self, d_in, d_out, n_frames: int, H: int, W: int, stream=None):
        from ._lib import lib

        assert 1 <= n_frames <= self.batch and (H, W) == (self.H, self.W)
        k = self._by_in[d_in.ptr]
        ctx, s, nbytes = self.ctx, self.ctx._s(stream), n_frames * H * W * 3
        for (_, op), out in zip(self._ops, self._outs[k]):
            if out is None:  # the member runs in its own slot buffers
                m_in, m_out = op.slot_buffers(k)
                ctx._check(lib.avx_memcpy_d2d(ctx._h, m_in.ptr, d_in.ptr, nbytes, s))
                op.run_device(m_in, m_out, n_frames, H, W, stream=s)
            else:
                op.run_device(d_in, out, n_frames, H, W, stream=s)
        Hc, Wc = self.layout.canvas_shape
        ctx._check(lib.avx_wall_compose_u8(ctx._h, self._layout_h, self._src[k], H * W * 3, n_frames, d_out.ptr, Hc * Wc * 3, s))

    def release_streams(self):
        for _, op in self._ops:
            release = getattr(op, "release_streams", None)
            if release is not None:
                release()

    def close(self):
        from ._lib import lib

        for _, op in self._ops:
            if hasattr(op, "close"):
                op.close()
        for outs in self._outs:
            for b in outs:
                if b is not None:
                    b.free()
        for pair in self._bufs:
            for b in pair:
                b.free()
        if self._layout_h:
            lib.avx_wall_layout_destroy(self.ctx._h, self._layout_h)
        self._ops, self._outs, self._bufs, self._src, self._layout_h = [], [], [], [], None


# ---------------------------------------------------------------- the command -----------------------
class _WallParser(argparse.ArgumentParser):
    """The command's parser; parse_args also resolves --species / --category and runs the `video` command's option checks."""

    def parse_args(self, args=None, namespace=None):
        from .video import check_io_options, check_raw_options

        args = super().parse_args(args, namespace)
        if (args.species is None) == (args.category is None):
            self.error("name the wall's species with exactly one of --species A,B,C and --category " + "|".join(CATEGORIES))
        if args.species is not None:
            names = [n.strip() for n in args.species.split(",") if n.strip()]
            if not names:
                self.error("--species names no species")
            unknown = [n for n in names if n not in _CLASS_NAMES]
            if unknown:
                self.error(f"--species: unknown species {', '.join(repr(n) for n in unknown)} (display names, e.g. Dog, HoneyBee, ReinDeer)")
            frame = per_frame_names(names)
            if frame:
                self.error(f"--species: {', '.join(frame)} run{'s' if len(frame) == 1 else ''} visualize() per frame and cannot stand on a wall")
        else:
            names = list(CATEGORIES[args.category])
            frame = per_frame_names(names)
            if frame:
                print(f"wall: --category {args.category}: dropped {', '.join(frame)} (no stream operator: they run visualize() per frame)", file=sys.stderr)
                names = [n for n in names if n not in frame]
        args.names = names
        if args.tile_height < 1 or args.pad < 0:
            self.error(f"--tile-height must be at least 1 and --pad at least 0 (got {args.tile_height} and {args.pad})")
        if len(names) + (0 if args.no_original else 1) > 64:
            self.error(f"a wall takes at most 64 tiles (got {len(names) + (0 if args.no_original else 1)})")
        check_io_options(self, args)
        check_raw_options(self, args)
        return args


def build_parser() -> argparse.ArgumentParser:
    from .video import add_input_options, add_io_arguments, add_output_options

    ap = _WallParser(prog="wall", description="Run several species on every frame of a video and write them side by side as one labelled grid.")
    add_io_arguments(ap)
    ap.add_argument("--species", default=None, metavar="A,B,C", help="display names separated by commas, e.g. Dog,Cat,HoneyBee,ReinDeer")
    ap.add_argument("--category", default=None, choices=list(CATEGORIES), help="every streamed species of a gallery category")
    ap.add_argument("--tile-height", type=int, default=256, help="height of a tile on the sheet (aspect kept)")
    ap.add_argument("--pad", type=int, default=8, help="pixels between and around the tiles")
    ap.add_argument("--no-labels", action="store_true", help="no label strip under the tiles")
    ap.add_argument("--no-original", action="store_true", help="do not show the input frame as the first tile")
    add_input_options(ap)
    add_output_options(ap)
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    if args.depth < 1:
        raise SystemExit("wall: --depth must be at least 1")
    from .pipeline import run_video
    from .renderers import VideoRenderer

    def renderer():
        return VideoRenderer(read_path=args.input, write_path=args.output, window_name="AnimalCam", matrix=args.matrix, range=args.range,
                             pix_fmt=args.pix_fmt, size=args.size, write_pix_fmt=args.out_pix_fmt, transfer=args.transfer, tonemap=args.tonemap,
                             peak_nits=args.peak_nits, sdr_white=args.sdr_white, out_matrix=args.out_matrix, scale=args.scale)

    try:
        vr = renderer()
        vr.open()
    except ValueError as e:
        if args.scale is None or "scale" not in str(e):
            raise
        raise SystemExit(f"wall: --scale {args.scale[0]}x{args.scale[1]}: {e}")  # a .y4m header smaller than --scale
    t0 = time.perf_counter()
    frames = 0
    try:
        hw = None if vr.y4m_header is None else (vr.y4m_header.height, vr.y4m_header.width)
        if args.size is not None:
            hw = (args.size[1], args.size[0])
        if hw is not None and args.scale is not None:
            hw = (args.scale[1], args.scale[0])  # what the species run on
        if hw is None:  # synthetic:, .npy or an image directory: peek at the size the wall is built for, then start over
            first = vr.get_image()
            hw = None if first is None else first.shape[:2]
            vr.close()
            vr = renderer()
            vr.open()
        if hw is not None:
            members = [(n, species_class(n)()) for n in args.names]
            try:
                op = WallStreamOp(members, hw[0], hw[1], tile_height=args.tile_height, pad=args.pad, labels=not args.no_labels,
                                  original=not args.no_original, depth=args.depth, batch=args.batch)
            except ValueError as e:
                raise SystemExit(f"wall: {e}")
            try:
                vr.set_output_size(*op.out_shape(hw[0], hw[1]))  # also the header of a sink that no frame reaches
                frames = run_video(op, vr, depth=args.depth, labels=None, batch=args.batch).frames
            finally:
                op.close()
    finally:
        vr.close()
    dt = time.perf_counter() - t0
    print(f"wall: {len(args.names)} species: {frames} frames in {dt:.2f} s ({frames / dt if dt > 0 else 0.0:.1f} fps)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
