"""What the pair commands -- `compare`, `diff`, `deltae` -- share: how A and B are named, checked and
opened, the device loop that walks their common prefix batch by batch, the map outputs of `diff` and `deltae` on top of it, the
output sink, and the tail of `main` that turns what was found into an exit status.

The loop (stream_pairs): `--depth` buffer sets (two where the command takes no --depth), each with a stream of its own, alternate:
the upload of batch i + 1 overlaps the kernels of batch i.  A command hands it one function, prepare(H, W), called once when the
frame size is known; it refuses a size the command cannot work on (SystemExit) and returns what differs between the commands:
  outputs  the per-set device outputs, each (bytes per frame, whether it is downloaded);
  enqueue(k, n, stream, sides, outs)  launches the command's kernels for the n frames of set k: sides[0] and sides[1] hold A and B
           (Side.d_rgb[k], or Side.d_in[k] for payloads as stored), outs the set's output buffers in the order of `outputs`;
  harvest(n, arrays)  the items of n finished frames from the set's staging arrays (None for an output that is not downloaded).
           The staging is filled again by a later batch: an item keeps a copy, never a view."""
from __future__ import annotations

import argparse
import itertools
import math
import os
import sys
from typing import Callable, Iterator, Optional, Sequence, Tuple

import numpy as np

from .runtime import get_context
from .video import _size_arg, check_io_options, check_raw_options


def num(v: float) -> str:
    return "inf" if math.isinf(v) else ("nan" if math.isnan(v) else f"{v:.6f}")


# ------------------------------------------------------------------------------------------------ the command line
def named_size(args, path: str) -> Optional[Tuple[int, int]]:
    """(W, H) of `path`'s frames where the command line states it: --size, or a synthetic: input."""
    if args.size is not None:
        return args.size
    if path.startswith("synthetic:"):
        try:
            return _size_arg(path.split(":")[1])
        except (IndexError, argparse.ArgumentTypeError):
            return None
    return None


def add_inputs(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("a", metavar="A", help=".y4m file, raw video (--pix-fmt), synthetic:<W>x<H>:<n>[:kind], .npy or an image directory")
    ap.add_argument("b", metavar="B", help="the same forms; the input options apply to both")


def check_stdin(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    if args.a == "-" and args.b == "-":
        ap.error("A and B cannot both be stdin")


def check_depth(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    if not 1 <= args.depth <= 8:
        ap.error(f"--depth must be 1..8 buffer sets (got {args.depth})")


def check_inputs(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """The input options of `video` with their defaults filled in, and a --scale that enlarges neither input."""
    args.input = args.a  # what check_io_options reads the source size of a synthetic: input from
    check_io_options(ap, args)
    check_raw_options(ap, args)
    for path in (args.a, args.b):
        src = named_size(args, path)
        if args.scale is not None and src is not None and (args.scale[0] > src[0] or args.scale[1] > src[1]):
            ap.error(f"--scale {args.scale[0]}x{args.scale[1]} enlarges the {src[0]}x{src[1]} source: --scale only reduces")


# ------------------------------------------------------------------------------------------------ the output
def sink_format(args) -> Optional[str]:
    """What OUT takes: "i420" (a .y4m sink), a raw pixel format name, or None for RGB frames (.npy, a PNG directory) and for no OUT."""
    from .renderers.video import is_raw_sink, is_y4m

    if args.out is None:
        return None
    fmt = args.out_pix_fmt
    if fmt is None and args.pix_fmt is not None and is_raw_sink(args.out):
        fmt = args.pix_fmt
    if fmt is not None:
        return fmt
    return "i420" if is_y4m(args.out) else None


def out_matrix(args) -> str:
    return args.out_matrix or ("bt709" if args.transfer is not None else args.matrix)


def open_sink(args, fmt: Optional[str], info: dict):
    """The opened renderer that writes args.out, taking what sink_format named `fmt`; info["hw"] sizes the payloads."""
    from .renderers import VideoRenderer

    sink = VideoRenderer(read_path=None, write_path=args.out, write_pix_fmt=None if fmt in (None, "i420") else fmt, matrix=out_matrix(args),
                         range=args.range, out_matrix=out_matrix(args))
    sink.open()
    if fmt is not None and "hw" in info:
        sink.set_output_size(*info["hw"])  # payloads name no size of their own
    return sink


def opened(items: Iterator) -> Iterator:
    """`items` with its first item drawn: the inputs are opened and their sizes checked before anything is written."""
    head = list(itertools.islice(items, 1))
    return itertools.chain(head, items)


def exit_status(name: str, args, info: dict, frames: int, first_bad: Optional[tuple] = None) -> int:
    """The tail of a command: 2 for inputs of different lengths without --shortest, 1 -- which outranks it -- for first_bad, the
    (frame, what it violates) of the first frame beyond a limit; each with its line on stderr."""
    status = 0
    if info.get("longer") and not args.shortest:
        print(f"{name}: {info['longer']} has more frames than the other input: compared the first {frames} (--shortest accepts that)", file=sys.stderr)
        status = 2
    if first_bad is not None:
        print(f"{name}: frame {first_bad[0]}: {first_bad[1]}", file=sys.stderr)
        status = 1
    return status


# ------------------------------------------------------------------------------------------------ the inputs
def _renderer(args, path: str):
    from .renderers import VideoRenderer

    if getattr(args, "planes", "rgb") == "yuv":
        raw = not path.lower().endswith(".y4m") and args.pix_fmt is not None
        return VideoRenderer(read_path=path, write_path=None, pix_fmt=args.pix_fmt if raw else None, size=args.size if raw else None)
    return VideoRenderer(read_path=path, write_path=None, matrix=args.matrix, range=args.range, pix_fmt=args.pix_fmt, size=args.size,
                         transfer=args.transfer, tonemap=args.tonemap, peak_nits=args.peak_nits, sdr_white=args.sdr_white, scale=args.scale)


def is_raw_input(args, path: str) -> bool:
    """Whether `path` is read as raw video with --pix-fmt and --size: every input that is not of a form that names itself -- a .y4m
    or .npy file, synthetic:, an image directory."""
    return args.pix_fmt is not None and not (path.lower().endswith((".y4m", ".npy")) or path.startswith("synthetic:") or os.path.isdir(path))


def open_source(args, path: str, renderer: Optional[Callable] = None):
    """The opened renderer of `path` and the (H, W) of the frames it will be compared at; renderer(args, path) makes it (default: the
    input options applied to every input alike)."""
    make = renderer or _renderer
    vr = make(args, path)
    vr.open()
    hw = vr.out_hw
    if hw is None:  # synthetic:, .npy or an image directory: peek at the first frame, then start over
        first = vr.get_image()
        hw = None if first is None else tuple(first.shape[:2])
        vr.close()
        vr = make(args, path)
        vr.open()
    return vr, hw


def copy(ctx, kind: str, dst, src, nbytes: int, stream) -> None:
    """Every copy of the loop, asynchronous on `stream`: kind "h2d" (staging to device buffer) or "d2h" (back)."""
    from ._lib import lib

    ctx._check(getattr(lib, "avx_memcpy_" + kind)(ctx._h, dst.ptr, src.ptr, nbytes, stream))


class Side:
    """One input: its staging (pinned) and device buffers, one of each per buffer set.  An input that hands over payloads (.y4m or
    raw SDR video without --scale) sends those across and decodes them into d_rgb on the device; with stored=True (--planes yuv)
    payloads are all it takes, d_in holds them as they are stored and there is no d_rgb.  hdr=True (`deltae --itp`) keeps both: the
    HDR payloads as stored in d_in, which the kernel reads, and -- with panel=True, for a map -- their tone-mapped decode in d_rgb."""

    def __init__(self, ctx, vr, H: int, W: int, batch: int, sets: int, name: str, stored: bool = False, hdr: bool = False, panel: bool = True):
        from .yuv import frame_size

        if stored and vr.yuv_hw is None:
            raise SystemExit(f"{name}: {vr.read_path}: --planes yuv needs a .y4m or raw video input")
        self.ctx, self.vr, self.H, self.W, self.name, self.stored, self.hdr = ctx, vr, H, W, name, stored, hdr
        self.payload = stored or hdr or (vr.yuv_hw is not None and vr.scale is None and vr.transfer is None)
        self.fmt = vr.yuv_pix_fmt or "yuv420p"  # a .y4m is I420
        self.unit = frame_size(self.fmt, H, W) if self.payload else H * W * 3
        self.host = [ctx.pinned((batch, self.unit), np.uint8) for _ in range(sets)]
        self.d_rgb = [] if stored or (hdr and not panel) else [ctx.malloc(batch * H * W * 3) for _ in range(sets)]
        self.d_in = [ctx.malloc(batch * self.unit) for _ in range(sets)] if self.payload else self.d_rgb

    def fill(self, k: int, limit: int) -> int:
        """Read up to `limit` frames into set k's staging; how many came."""
        n = 0
        while n < limit:
            f = self.vr.get_yuv() if self.payload else self.vr.get_image()
            if f is None:
                break
            f = np.asarray(f)
            if not self.payload and (f.dtype != np.uint8 or f.shape != (self.H, self.W, 3)):
                raise SystemExit(f"{self.name}: {self.vr.read_path}: frame {self.vr.last_index} is {f.dtype} {f.shape}, not uint8 {(self.H, self.W, 3)}")
            self.host[k].array[n] = f.reshape(-1)
            n += 1
        return n

    def enqueue(self, k: int, n: int, stream) -> None:
        """Upload set k's n staged frames and, where they are payloads to decode, decode them into d_rgb[k]."""
        copy(self.ctx, "h2d", self.d_in[k], self.host[k], n * self.unit, stream)
        if self.payload and self.d_rgb:
            self.vr.decode.launch(self.ctx, self.d_in[k], self.d_rgb[k], n, self.H, self.W, stream)

    def free(self) -> None:
        for b in self.d_rgb + (self.d_in if self.payload else []) + self.host:
            b.free()


# ------------------------------------------------------------------------------------------------ the device loop
def stream_pairs(args, info: dict, name: str, prepare: Callable, stored: bool = False, renderer: Optional[Callable] = None,
                 hdr: Sequence[bool] = (False, False), panels: bool = True) -> Iterator:
    """What `harvest` makes of the common prefix of args.a and args.b, in frame order (the module's docstring has prepare and what it
    returns).  `name` is the command's, for messages; `stored` compares payloads as stored (Side); renderer(args, path) opens an input
    (open_source); hdr names the inputs that are HDR sides, which keep their payloads, and panels whether those are also decoded (Side).
    info["longer"] names the input ("A" / "B") that had frames left over, when one had.  Buffers and streams are released however the
    generator ends."""
    how = {} if renderer is None else {"renderer": renderer}  # without one the call is open_source(args, path), as it was
    va, hwa = open_source(args, args.a, **how)
    vb, hwb = open_source(args, args.b, **how)
    ctx, sides, streams, bufs = None, [], [], []
    try:
        if hwa is not None and hwb is not None and tuple(hwa) != tuple(hwb):
            raise SystemExit(f"{name}: frame sizes differ: A is {hwa[1]}x{hwa[0]}, B is {hwb[1]}x{hwb[0]}")
        if hwa is None or hwb is None:  # an empty input
            if hwa is not None or hwb is not None:
                info["longer"] = "A" if hwa is not None else "B"
            return
        H, W = hwa
        outputs, enqueue, harvest = prepare(H, W)
        ctx, batch, sets = get_context(), args.batch, args.depth or 2
        for vr, is_hdr in zip((va, vb), hdr):
            sides.append(Side(ctx, vr, H, W, batch, sets, name, stored, is_hdr, panels))
        d_out, h_out = [[] for _ in range(sets)], [[] for _ in range(sets)]
        for k in range(sets):
            streams.append(ctx.stream_create())
            for nbytes, download in outputs:
                d_out[k].append(ctx.malloc(batch * nbytes))
                h_out[k].append(ctx.pinned((batch, nbytes), np.uint8) if download else None)
                bufs += [b for b in (d_out[k][-1], h_out[k][-1]) if b is not None]
        pending = [0] * sets

        def collect(k):
            ctx.sync(streams[k])
            n, pending[k] = pending[k], 0
            return harvest(n, [None if h is None else h.array for h in h_out[k]]) if n else []

        i = 0
        while True:
            k = i % sets
            yield from collect(k)  # the set's previous batch: its buffers are free again afterwards
            na, nb = sides[0].fill(k, batch), sides[1].fill(k, batch)
            n = min(na, nb)
            if n:
                for s in sides:
                    s.enqueue(k, n, streams[k])
                enqueue(k, n, streams[k], sides, d_out[k])
                for (nbytes, _), d, h in zip(outputs, d_out[k], h_out[k]):
                    if h is not None:
                        copy(ctx, "d2h", h, d, n * nbytes, streams[k])
                pending[k] = n
            i += 1
            if na != nb:
                info["longer"] = "A" if na > nb else "B"
            if n < batch:
                break
        for j in range(sets):
            yield from collect((i + j) % sets)
    finally:
        for s in streams:
            ctx.sync(s)
            ctx.stream_destroy(s)
        for b in bufs + sides:
            b.free()
        va.close()
        vb.close()


def stream_map_pairs(args, info: dict, name: str, fmt: Optional[str], launch: Callable, rec_bytes: int, records: Callable,
                     check_size: Optional[Callable] = None, renderer: Optional[Callable] = None, hdr: Sequence[bool] = (False, False),
                     launch_sides: bool = False) -> Iterator[Tuple[Optional[np.ndarray], object]]:
    """stream_pairs for a command that writes a map per pair (`diff`, `deltae`): (output frame, record) of every pair.  Without
    args.out the frame is None and there is no map.  Otherwise it is RGB uint8 H x W x 3 (H x 3W x 3 with --layout side) when fmt is
    None, else the flat payload the device encoded the map to ("i420", or a raw pixel format name).  info["hw"] is the output
    frames' (H, W) once the first item is there.  launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, stream) enqueues the command's
    kernel (d_map: None without a map); records(bytes, n) reads n records of rec_bytes; check_size(H, W) refuses a frame size.
    renderer and hdr are stream_pairs'; with launch_sides the kernel reads the sides as they are (`deltae --itp`: an HDR side's payloads)
    and launch is called as launch(ctx, sides, k, n, H, W, d_map, d_rec, stream) with the two Sides and the buffer set k."""
    from .yuv import Encode

    def prepare(H, W):
        if check_size is not None:
            check_size(H, W)
        with_map = args.out is not None
        Wo = 3 * W if args.layout == "side" else W
        info["hw"] = (H, Wo)
        encode = None if fmt is None else Encode(None if fmt == "i420" else fmt, out_matrix(args), args.range or "limited")
        unit = H * Wo * 3 if fmt is None else encode.frame_bytes(H, Wo)
        # the map (downloaded as it is where the sink takes RGB), the payload it is encoded to, the records
        outputs = ([(H * Wo * 3, fmt is None)] if with_map else []) + ([(unit, True)] if fmt is not None else []) + [(rec_bytes, True)]

        def enqueue(k, n, stream, sides, outs):
            ctx = sides[0].ctx
            if launch_sides:
                launch(ctx, sides, k, n, H, W, outs[0] if with_map else None, outs[-1], stream)
            else:
                launch(ctx, sides[0].d_rgb[k], sides[1].d_rgb[k], n, H, W, outs[0] if with_map else None, outs[-1], stream)
            if encode is not None:
                encode.launch(ctx, outs[0], outs[1], n, H, Wo, stream)

        def harvest(n, arrays):
            recs = records(arrays[-1], n)
            if not with_map:
                return [(None, r) for r in recs]
            shape = (H, Wo, 3) if fmt is None else (unit,)
            return [(np.array(arrays[-2][j]).reshape(shape), recs[j]) for j in range(n)]  # copies: the set is filled again

        return outputs, enqueue, harvest

    return stream_pairs(args, info, name, prepare, renderer=renderer, hdr=hdr, panels=args.out is not None)
