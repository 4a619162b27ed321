"""The frame loop (reference: main.py:53-72 `video`, one frame in flight, synchronous) as a pipelined,
sharded device loop.

  * Sharding: frames are independent, so frame i belongs to rank i mod world (round-robin,
    BASELINE.json config 4).  One process per GPU; NO collective on the data path.  torch.distributed
    (RCCL over xGMI on the GPU box, gloo in CPU tests) carries only the start/stop barriers and the
    reduction of per-rank statistics.
  * Pipelining inside a rank: `depth` slots, each with its own HIP stream, pinned host buffers and HBM
    buffers; a frame's H2D copy, kernels and D2H copy are enqueued in order on its slot's stream, so the
    copies of frames i+1 / i-1 overlap the kernels of frame i (different streams), and the host only
    blocks on a slot when it comes around again."""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Callable, Iterator, List, Optional, Tuple

import numpy as np


# ---------------------------------------------------------------- sharding (pure host logic) --------
def shard_indices(n_frames: int, rank: int, world: int) -> List[int]:
    """Global frame indices owned by `rank`: i mod world == rank."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world {world}")
    return list(range(rank, n_frames, world))


def owner_of(frame_index: int, world: int) -> int:
    return frame_index % world


def merge_in_order(per_rank: List[List[Tuple[int, object]]]) -> List[object]:
    """Re-interleave per-rank (index, item) lists into stream order; checks every index appears once."""
    flat = sorted((i, item) for lst in per_rank for i, item in lst)
    idx = [i for i, _ in flat]
    if idx != list(range(len(idx))):
        raise ValueError("frame indices are not a permutation of 0..n-1")
    return [item for _, item in flat]


@dataclass
class StreamStats:
    frames: int = 0
    pixels: int = 0
    seconds: float = 0.0
    ranks: int = 1
    host_copy_seconds: float = 0.0  # this rank's (after reduce_stats: the slowest rank's) time in pageable <-> pinned frame copies

    @property
    def megapixels_per_second(self) -> float:
        return self.pixels / 1e6 / self.seconds if self.seconds > 0 else 0.0


def reduce_stats(local: StreamStats, dist=None) -> StreamStats:
    """Whole-job statistics: frames and pixels summed over ranks, wall time = max over ranks."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return local
    import torch

    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    s = torch.tensor([float(local.frames), float(local.pixels)], dtype=torch.float64, device=dev)
    t = torch.tensor([local.seconds, local.host_copy_seconds], dtype=torch.float64, device=dev)
    dist.all_reduce(s, op=dist.ReduceOp.SUM)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return StreamStats(int(s[0].item()), int(s[1].item()), float(t[0].item()), dist.get_world_size(), float(t[1].item()))


# ---------------------------------------------------------------- device pipeline -------------------
# Host copies of a frame (pageable <-> pinned, 25 MB at 4K) run on a few threads: one core moves ~10 GB/s and faults the fresh
# output array's pages in one by one, which made the host side of a dichromat stream (2 ms per 4K frame) the limiter, not the GPU.
_COPY_THREADS = 4
_copy_pool = None


def _pcopy(dst: np.ndarray, src: np.ndarray) -> None:
    """dst[...] = src, split by rows over a small thread pool for large frames (NumPy releases the GIL while copying)."""
    global _copy_pool
    if src.nbytes < (4 << 20) or src.shape[0] < _COPY_THREADS:
        dst[...] = src
        return
    if _copy_pool is None:
        from concurrent.futures import ThreadPoolExecutor

        _copy_pool = ThreadPoolExecutor(max_workers=_COPY_THREADS, thread_name_prefix="avx-copy")
    rows = src.shape[0]
    step = (rows + _COPY_THREADS - 1) // _COPY_THREADS

    def part(r0):
        dst[r0:r0 + step] = src[r0:r0 + step]

    list(_copy_pool.map(part, range(0, rows, step)))


@dataclass
class _Slot:
    stream: int
    h_in: object
    h_out: object
    d_in: object
    d_out: object
    index: int = -1
    busy: bool = False
    indices: List[int] = field(default_factory=list)  # global indices of the frames the slot carries (<= batch)
    d_yuv_in: object = None   # io_format="i420" / "yuv": the frame's payload on the device, in and out
    d_yuv_out: object = None
    d_left: object = None     # the left half of the split frame: d_in, or the op's baseline (split_baseline)
    d_full: object = None     # scale= with io_format="rgb": the source-size RGB frames that avx_resize_hwc reduces into d_in


class FramePipeline:
    """Runs `op.run_device(d_in, d_out, n, H, W, stream=...)` (DichromatOp / HoneybeeOp / SpeciesStreamOp) over a stream of
    uint8 frames with `depth` slots in flight, each carrying up to `batch` frames (n = batch, or what is left at the end)."""

    def __init__(self, op, H: int, W: int, *, ctx=None, depth: int = 3, split_compare: bool = False, draw_seam: bool = True,
                 labels: Optional[Tuple[Optional[str], Optional[str]]] = ("Original", "Transformed"), io_format: str = "rgb",
                 matrix: str = "bt601", yuv_range: str = "limited", split_baseline: bool = False, batch: int = 1,
                 pix_fmt: Optional[str] = None, transfer: Optional[str] = None, tonemap: str = "mobius", peak_nits: float = 1000.0,
                 sdr_white: float = 203.0, out_matrix: Optional[str] = None, scale: Optional[Tuple[int, int]] = None, decode=None, encode=None):
        """split_compare: emit make_split_frame(original, transformed) composed on the device (renderers/video.py:198-245:
        halves, seam, and the two corner labels -- `labels` = (left, right), None = none) instead of the transformed frame.

        io_format: "rgb" -- frames in and out are HxWx3 uint8; "i420" -- they are flat I420 payloads (the Y4M layout, 1.5 B/px:
        half the bytes of the host and PCIe copies), converted on the slot stream into the op's d_in and back out of its
        d_out (yuv.py, with `matrix` and `yuv_range`); the op, the split composition and the labels run on RGB as before;
        "yuv" -- as "i420", with flat payloads in the raw pixel format `pix_fmt` (one of yuv.PIX_FMTS: nv12, p010le, ...; DESIGN
        §4.9) and the conversions of csrc/yuv_raw.hip.  Format names go in `pix_fmt`, not in io_format.

        transfer: "pq" or "hlg" -- the payloads are HDR (BT.2020, 10-bit `pix_fmt`, io_format="yuv"): the slot stream decodes
        them with `tonemap`, `peak_nits` and `sdr_white` instead of `matrix`, and the op sees tone-mapped SDR frames.
        The output side is SDR: it is encoded in `out_matrix`, which defaults to "bt709" with a transfer and to `matrix` without
        one.  With transfer=None nothing else changes.

        scale: (Wd, Hd), in the order of the video command's --size -- frames are read at H x W and reduced to Hd x Wd (cv2's
        INTER_AREA; never enlarged) on the slot stream before the op sees them.  H, W stay the source size; the
        slot's RGB buffers, the op, the split composition, the labels and everything on the way out (`out_H`, `out_W`, the
        emitted frames or payloads) have the scaled size.  io_format="yuv" / "i420" decode straight to the scaled frame
        (with a `transfer` §4.13: one launch per slot, no full-size RGB frame); io_format="rgb" frames land in a
        source-size buffer of the slot and go through avx_resize_hwc frame by frame.  With scale=None nothing changes.

        decode, encode: a yuv.Decode and a yuv.Encode, in place of all the format keywords above (naming both is refused).  The
        keywords are turned into the same pair (yuv.codec); `decode` and `encode` hold it, and their launch() is what the slot stream
        runs, so which C entry point a combination reaches is decided in yuv.py alone.

        split_baseline: the split frame's left half is the op's own baseline -- `op.slot_baseline(k)`, the frame a species'
        visualize() returns first (a UV species' panorama-warped input, SpeciesStreamOp) -- instead of the input frame.

        batch: frames per slot.  A slot's pinned staging and device buffers hold `batch` contiguous frames: one H2D copy, one
        op.run_device(..., n, ...), the split composition and labels per frame, the I420 conversions over the n frames, one D2H
        copy.  Frames are still emitted one by one in submission order; the last slot of a stream may carry fewer frames.  The
        op states how many frames one call takes in `max_batch` (absent: 1); an op that cannot take `batch` is refused here.

        An op whose output is not the size of its input says so with `out_shape(H, W) -> (Hc, Wc)` (wall.WallStreamOp: the labelled
        grid of several species): the slot's d_out, the pinned output staging, the encode and the emitted frames or
        payloads then have that size, and so have `out_H` / `out_W`; `op_H` / `op_W` name what the op is handed, and StreamStats
        still counts those pixels.  split_compare composes two frames of one size: with such an op it is refused.  An op without
        out_shape changes nothing here."""
        from .runtime import get_context
        from .yuv import PIX_FMTS, codec

        if decode is not None or encode is not None:
            import inspect

            given = dict(io_format=io_format, pix_fmt=pix_fmt, matrix=matrix, yuv_range=yuv_range, transfer=transfer, tonemap=tonemap,
                         peak_nits=peak_nits, sdr_white=sdr_white, out_matrix=out_matrix, scale=scale)
            defaults = inspect.signature(FramePipeline.__init__).parameters
            named = [k for k, v in given.items() if v != defaults[k].default]
            if named or decode is None or encode is None:
                raise ValueError("decode= and encode= go together and take the place of the format keywords "
                                 f"(got {', '.join(named) or 'one of the two'})")
            io_format, pix_fmt = ("i420" if decode.pix_fmt is None else "yuv"), decode.pix_fmt
        else:
            if io_format not in ("rgb", "i420", "yuv"):
                raise ValueError(f"io_format must be 'rgb', 'i420' or 'yuv' (got {io_format!r})")
            if io_format == "yuv" and pix_fmt not in PIX_FMTS:
                raise ValueError(f"io_format='yuv' needs pix_fmt, one of {', '.join(PIX_FMTS)} (got {pix_fmt!r})")
            if io_format != "yuv" and pix_fmt is not None:
                raise ValueError(f"pix_fmt goes with io_format='yuv' (got io_format={io_format!r})")
            if transfer is not None and io_format != "yuv":
                raise ValueError(f"transfer={transfer!r} goes with io_format='yuv' and a 10-bit pix_fmt (got io_format={io_format!r})")
            # io_format="rgb" holds the pair too: its settings are checked all the same, and its Decode carries the scale
            decode, encode = codec(pix_fmt, matrix, yuv_range, transfer, tonemap, peak_nits, sdr_white, out_matrix, scale)
        self.decode, self.encode, self.io_format, self.pix_fmt = decode, encode, io_format, pix_fmt
        self.matrix, self.yuv_range, self.out_matrix = decode.matrix, decode.range, encode.matrix
        self.transfer, self.tonemap, self.peak_nits, self.sdr_white = decode.transfer, decode.tonemap, float(decode.peak_nits), float(decode.sdr_white)
        self.op, self.H, self.W, self.depth = op, H, W, depth
        self.op_H, self.op_W = decode.out_hw(H, W)  # what the op is handed
        self.scale = scale = None if decode.scale is None else (self.op_W, self.op_H)
        shape_of = getattr(op, "out_shape", None)
        if shape_of is not None and split_compare:
            raise ValueError(f"split_compare: {type(op).__name__}'s output has a size of its own (out_shape); there is no frame to compare it with")
        self.out_H, self.out_W = (int(v) for v in shape_of(self.op_H, self.op_W)) if shape_of is not None else (self.op_H, self.op_W)
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"batch must be at least 1 (got {batch})")
        cap = getattr(op, "max_batch", 1)
        if self.batch > 1 and self.batch > cap:
            raise ValueError(f"batch={self.batch}: {type(op).__name__} takes at most {cap} frame(s) per call")
        self.split_compare, self.draw_seam = bool(split_compare), bool(draw_seam)
        baseline = getattr(op, "slot_baseline", None) if split_baseline else None
        if split_baseline and baseline is None:
            raise ValueError(f"split_baseline: {type(op).__name__} has no slot_baseline(k)")
        self.labels = tuple(labels) if labels else (None, None)
        self.ctx = ctx or getattr(op, "ctx", None) or get_context()
        if getattr(op, "ctx", None) is None:
            op.ctx = self.ctx
        iH, iW, oH, oW = self.op_H, self.op_W, self.out_H, self.out_W
        nbytes, out_nbytes = iH * iW * 3 * self.batch, oH * oW * 3 * self.batch
        # ops that own their device frames (recorded species plans, animals/_uv_species.py::SpeciesStreamOp) lend them per slot
        lend = getattr(op, "slot_buffers", None)
        self._lent = lend is not None
        self.slots = []
        if io_format == "rgb":
            self._in_shape, self._io_shape = (H, W, 3), (oH, oW, 3)  # frames in (source size), frames out
        else:
            self._in_shape, self._io_shape = (decode.frame_bytes(H, W),), (encode.frame_bytes(oH, oW),)
        full = scale is not None and io_format == "rgb"
        for k in range(depth):
            d_in, d_out = lend(k) if lend else (self.ctx.malloc(nbytes), self.ctx.malloc(out_nbytes))
            if d_in.nbytes < nbytes or d_out.nbytes < out_nbytes:
                raise ValueError(f"batch={self.batch}: {type(op).__name__}'s slot buffers hold fewer than {self.batch} frames")
            s = _Slot(self.ctx.stream_create(), self.ctx.pinned((self.batch,) + self._in_shape, np.uint8),
                      self.ctx.pinned((self.batch,) + self._io_shape, np.uint8), d_in, d_out)
            s.d_left = baseline(k) if baseline is not None else d_in
            if io_format != "rgb":
                s.d_yuv_in, s.d_yuv_out = self.ctx.malloc(self.batch * self._in_shape[0]), self.ctx.malloc(self.batch * self._io_shape[0])
            if full:
                s.d_full = self.ctx.malloc(self.batch * H * W * 3)
            self.slots.append(s)

    def close(self):
        for s in self.slots:
            self.ctx.sync(s.stream)
        release = getattr(self.op, "release_streams", None)  # ops that wrap the slot streams (ml/predict.py::MstHoneybeeStreamOp) drop the wrappers first
        if release is not None:
            release()
        for s in self.slots:
            self.ctx.stream_destroy(s.stream)
            s.h_in.free(); s.h_out.free()
            if not self._lent:
                s.d_in.free(); s.d_out.free()
            if s.d_yuv_in is not None:
                s.d_yuv_in.free(); s.d_yuv_out.free()
            if s.d_full is not None:
                s.d_full.free()
        self.slots = []

    def _retire(self, s: _Slot, emit: Callable[[int, np.ndarray], None]):
        if s.busy:
            self.ctx.sync(s.stream)
            for j, index in enumerate(s.indices):
                t0 = time.perf_counter()
                out = np.empty(self._io_shape, np.uint8)
                _pcopy(out, s.h_out.array[j])
                self._copy_s += time.perf_counter() - t0
                emit(index, out)
            s.busy, s.indices = False, []

    def run(self, frames: Iterator[Tuple[int, np.ndarray]], emit: Callable[[int, np.ndarray], None]) -> StreamStats:
        """frames: (global index, HxWx3 uint8 -- or, io_format="i420" / "yuv", a flat payload) pairs owned by this rank;
        emit(index, out) in submission order, `out` in the same format."""
        from ._lib import lib

        ctx, n, t0 = self.ctx, 0, time.perf_counter()
        self._copy_s = 0.0
        for s in self.slots:  # a run that ended in an error may have left a half-filled slot behind
            s.busy, s.indices = False, []
        i420 = self.io_format != "rgb"  # payloads cross the host and PCIe; RGB exists on the device only
        iH, iW, oH, oW = self.op_H, self.op_W, self.out_H, self.out_W  # the op's input (the scaled frame), its output
        src_rgb_bytes = self.H * self.W * 3

        def reduce_full(s, m):
            """scale=: the m source-size frames of s.d_full -> s.d_in, cv2's INTER_AREA, frame by frame on the slot's stream."""
            for f in range(m):
                ctx._check(lib.avx_resize_hwc(ctx._h, s.d_full.ptr + f * src_rgb_bytes, 2, self.H, self.W, 3, s.d_in.ptr + f * iH * iW * 3, iH, iW, 3,
                                              s.stream))

        in_bytes, fbytes = int(np.prod(self._in_shape)), int(np.prod(self._io_shape))
        rgb_bytes = oH * oW * 3

        def submit(s: _Slot):
            """Everything one slot's frames need, in order on the slot's stream."""
            m = len(s.indices)
            if i420:
                ctx._check(lib.avx_memcpy_h2d(ctx._h, s.d_yuv_in.ptr, s.h_in.ptr, m * in_bytes, s.stream))
                self.decode.launch(ctx, s.d_yuv_in, s.d_in, m, self.H, self.W, s.stream)
            elif self.scale is not None:
                ctx._check(lib.avx_memcpy_h2d(ctx._h, s.d_full.ptr, s.h_in.ptr, m * in_bytes, s.stream))
                reduce_full(s, m)
            else:
                ctx._check(lib.avx_memcpy_h2d(ctx._h, s.d_in.ptr, s.h_in.ptr, m * in_bytes, s.stream))
            self.op.run_device(s.d_in, s.d_out, m, iH, iW, stream=s.stream)
            if self.split_compare:
                for f in range(m):
                    o = f * rgb_bytes
                    ctx._check(lib.avx_split_compose_u8(ctx._h, s.d_left.ptr + o, s.d_out.ptr + o, s.d_out.ptr + o, oH, oW, int(self.draw_seam), s.stream))
                    if self.labels[0] is not None or self.labels[1] is not None:
                        from .renderers.labels import draw_split_labels_device

                        draw_split_labels_device(ctx, s.d_out.ptr + o, oH, oW, self.labels[0], self.labels[1], s.stream)
            if i420:
                self.encode.launch(ctx, s.d_out, s.d_yuv_out, m, oH, oW, s.stream)
                ctx._check(lib.avx_memcpy_d2h(ctx._h, s.h_out.ptr, s.d_yuv_out.ptr, m * fbytes, s.stream))
            else:
                ctx._check(lib.avx_memcpy_d2h(ctx._h, s.h_out.ptr, s.d_out.ptr, m * fbytes, s.stream))
            s.index, s.busy = s.indices[0], True

        k, s = 0, None  # slots submitted so far; the slot being filled
        for index, frame in frames:
            if s is None:
                s = self.slots[k % self.depth]
                self._retire(s, emit)
            if frame.shape != self._in_shape or frame.dtype != np.uint8:
                raise ValueError(f"frame {index}: expected uint8 {self._in_shape}, got {frame.dtype} {frame.shape}")
            tc = time.perf_counter()
            _pcopy(s.h_in.array[len(s.indices)], frame)
            self._copy_s += time.perf_counter() - tc
            s.indices.append(index)
            n += 1
            if len(s.indices) == self.batch:
                submit(s)
                k, s = k + 1, None
        if s is not None and s.indices:  # the stream's last, partial batch
            submit(s)
            k += 1
        for j in range(self.depth):  # drain in submission order
            self._retire(self.slots[(k + j) % self.depth], emit)
        return StreamStats(n, n * iH * iW, time.perf_counter() - t0, 1, self._copy_s)  # pixels the op saw


def run_video(animal_op, renderer, *, rank: int = 0, world: int = 1, depth: int = 3, split_compare: bool = False, dist=None,
              labels: Optional[Tuple[Optional[str], Optional[str]]] = ("Original", "Transformed"), split_baseline: bool = False,
              batch: int = 1) -> StreamStats:
    """main.py:53-72 on the device: read -> visualize -> (split-compose + labels) -> render, this rank's shard only.

    A renderer that shards itself (renderers.VideoRenderer(rank=, world=): strided source, index-addressed sink) hands over
    only this rank's frames and its `last_index` names each one's place in the stream; any other get_image()/render() pair
    is read in full and filtered here (frame i belongs to rank i mod world).  Outputs go to the sink under their GLOBAL frame
    index; after the ranks' closing collective (the statistics reduction) rank 0 reassembles a sharded .npy sink into the one
    ordered stream ("host re-orders outputs by frame index before render()").

    A renderer whose frames can stay I420 end to end (`yuv_hw` not None: renderers.VideoRenderer from a .y4m to a .y4m) hands
    over get_yuv() payloads, and the pipeline runs with the renderer's own `decode` and `encode` (yuv.Decode, yuv.Encode): I420, or the
    raw pixel format the renderer names (raw video in and out in one format), with its HDR settings when it has
    them.  A renderer with a `scale` hands its payloads over at the source size and the pipeline reduces them as it decodes
    (DESIGN §4.11); the frames get_image() returns are scaled already.
    split_baseline, batch (frames per slot and per op call): see FramePipeline.  Where the op has an output size of its own
    (FramePipeline: out_shape) the renderer is told so (set_output_size) before the first frame is rendered."""
    self_sharding = getattr(renderer, "world", 1) == world and getattr(renderer, "rank", 0) == rank and hasattr(renderer, "last_index") and world > 1
    yuv_hw = getattr(renderer, "yuv_hw", None) if callable(getattr(renderer, "get_yuv", None)) else None
    get = renderer.get_yuv if yuv_hw is not None else renderer.get_image
    first = get()
    if first is None:
        stats = StreamStats()
        pipe = None
    elif yuv_hw is not None:
        H, W = yuv_hw
        pipe = FramePipeline(animal_op, H, W, depth=depth, split_compare=split_compare, labels=labels, split_baseline=split_baseline, batch=batch,
                             decode=renderer.decode, encode=renderer.encode)
    else:
        H, W, _ = first.shape
        pipe = FramePipeline(animal_op, H, W, depth=depth, split_compare=split_compare, labels=labels, split_baseline=split_baseline, batch=batch)

    if pipe is not None and (pipe.out_H, pipe.out_W) != (pipe.op_H, pipe.op_W) and hasattr(renderer, "set_output_size"):
        renderer.set_output_size(pipe.out_H, pipe.out_W)  # an op with out_shape: the sinks take the pipeline's output size, not the input's

    def frames():
        i, f = 0, first
        while f is not None:
            if self_sharding:
                yield renderer.last_index, f
            elif owner_of(i, world) == rank:
                yield i, f
            i += 1
            f = get()

    def emit(i, out):
        if self_sharding:
            renderer.render(out, index=i)  # already split-composed on the device when split_compare
        else:
            renderer.render(out)

    if pipe is not None:
        try:
            stats = pipe.run(frames(), emit)
        finally:
            pipe.close()
    if hasattr(renderer, "flush"):
        renderer.flush()
    total = reduce_stats(stats, dist)  # a collective: every rank's shard is flushed once it returns anywhere
    if world > 1 and rank == 0 and dist is not None and hasattr(renderer, "merge_shards"):
        renderer.close()
        renderer.merge_shards()
    return total
