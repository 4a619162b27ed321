"""The `compare` command: PSNR, SSIM and code differences of two videos, frame by frame, on the device:

    python -m animal_vision_amd.compare full.y4m half.y4m --csv quality.csv
    python -m animal_vision_amd.compare a.yuv b.yuv --pix-fmt nv12 --size 3840x2160 --max-abs 1 --max-beyond1 0.002
    python -m animal_vision_amd.compare a.yuv b.yuv --pix-fmt p010le --size 3840x2160 --planes yuv --max-abs 1

A and B are any two source forms of renderers.VideoRenderer (.y4m, raw video with --pix-fmt and --size, .npy, an image directory,
synthetic:); the input-side options of `video` (--pix-fmt, --size, --matrix, --range, --transfer and its options, --scale) apply to
both.  Frames are compared as a species of `video` would see them: RGB uint8 after decode, tone map and scale.  An input that hands
over payloads (a .y4m or raw SDR input without --scale) sends them across PCIe and is decoded by yuv.py's device functions into the
batch buffer; every other input's get_image() frames are uploaded.  Two buffer sets, each with a stream of its own, alternate: the
upload of batch i + 1 overlaps the kernel of batch i.

One CSV line per frame goes to stdout (or --csv FILE): frame,psnr_r,psnr_g,psnr_b,psnr,ssim_r,ssim_g,ssim_b,ssim,max_abs,beyond1
(beyond1: the share of samples more than one code apart).  A summary line goes to stderr.  --min-psnr, --min-ssim, --max-abs and
--max-beyond1 make the command a check: status 1 when a frame violates one (the first such frame is named on stderr).  Inputs of
different frame sizes are an error before any frame is compared; of different lengths, the common prefix is compared and the status
is 2 unless --shortest is given.

--planes yuv compares video in its own Y, U and V planes instead: both inputs hand over payloads (.y4m, or raw video with
--pix-fmt and --size; a .y4m is I420 whatever --pix-fmt says), which go into the batch buffers and straight to avx_plane_metrics -- no
decode, no RGB buffer, 10-bit files in 10-bit codes.  The lines are frame,psnr_y,psnr_u,psnr_v,psnr,ssim_y,ssim_u,ssim_v,ssim,max_abs,
beyond1 (psnr: pooled over all samples, ffmpeg's `average`; ssim: the planes weighted by their sample counts; absent planes: nan).

--ms-ssim adds MS-SSIM over five scales (Wang, Simoncelli, Bovik 2003) of the RGB frames: the columns ms_ssim_r,
ms_ssim_g,ms_ssim_b,ms_ssim behind the others (which stay, byte for byte, what the run without it prints), mean and minimum in the
summary, and --min-ms-ssim X as a limit (it implies --ms-ssim).  Five scales need frames of at least 176 x 176 (after --scale);
--no-ssim and --planes yuv are refused with it."""
from __future__ import annotations

import argparse
import itertools
import math
import os
import sys
import time
from typing import Iterator, Optional, Sequence

import numpy as np

from .metrics import (MS_MIN_SIDE, MS_RECORD_BYTES, PLANE_RECORD_BYTES, RECORD_BYTES, FrameMetrics, MsSsim, PlaneMetrics, _psnr,
                      check_plane_formats, frame_metrics_launch, frame_metrics_ms_launch, ms_records_from_bytes, plane_metrics_launch,
                      plane_records_from_bytes, records_from_bytes)
from .video import _size_arg, add_input_options, add_output_options, check_io_options, check_raw_options

CSV_HEADER = "frame,psnr_r,psnr_g,psnr_b,psnr,ssim_r,ssim_g,ssim_b,ssim,max_abs,beyond1"
CSV_HEADER_YUV = "frame,psnr_y,psnr_u,psnr_v,psnr,ssim_y,ssim_u,ssim_v,ssim,max_abs,beyond1"
CSV_MS_COLUMNS = ",ms_ssim_r,ms_ssim_g,ms_ssim_b,ms_ssim"  # --ms-ssim: behind CSV_HEADER
_OUTPUT_ONLY = (("--out-pix-fmt", "out_pix_fmt"), ("--out-matrix", "out_matrix"), ("--depth", "depth"))


def _num(v: float) -> str:
    return "inf" if math.isinf(v) else ("nan" if math.isnan(v) else f"{v:.6f}")


def format_row(index: int, m: FrameMetrics) -> str:
    """The CSV line of frame `index`."""
    p = m.psnr_channels
    return ",".join([str(index), _num(p[0]), _num(p[1]), _num(p[2]), _num(m.psnr), _num(m.ssim[0]), _num(m.ssim[1]), _num(m.ssim[2]),
                     _num(m.ssim_mean), str(m.max_abs), f"{m.share_beyond(1):.6g}"])


def format_row_planes(index: int, m: PlaneMetrics) -> str:
    """The CSV line of frame `index` with --planes yuv."""
    p = m.psnr_planes
    return ",".join([str(index), _num(p[0]), _num(p[1]), _num(p[2]), _num(m.psnr), _num(m.ssim[0]), _num(m.ssim[1]), _num(m.ssim[2]),
                     _num(m.ssim_mean), str(m.max_abs), f"{m.share_beyond(1):.6g}"])


def format_ms_columns(ms: MsSsim) -> str:
    """What --ms-ssim appends to the CSV line of a frame."""
    c = ms.ms_ssim_channels
    return "," + ",".join([_num(c[0]), _num(c[1]), _num(c[2]), _num(ms.ms_ssim)])


def _is_y4m_file(path: str) -> bool:
    return path.lower().endswith(".y4m")


def plane_format(args, path: str) -> str:
    """The pixel format `path` hands its payloads over in with --planes yuv: a .y4m file (and stdin without --pix-fmt) is I420."""
    return "yuv420p" if _is_y4m_file(path) or args.pix_fmt is None else args.pix_fmt


def _check_planes_yuv(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """--planes yuv: payloads as stored, so nothing that works on RGB, and two formats of one depth and subsampling."""
    if args.scale is not None:
        ap.error("--scale reduces RGB frames: --planes yuv compares the planes as stored")
    for flag, v in (("--transfer", args.transfer), ("--tonemap", args.tonemap), ("--peak-nits", args.peak_nits), ("--sdr-white", args.sdr_white)):
        if v is not None:
            ap.error(f"{flag} tone-maps to SDR RGB: --planes yuv compares HDR files as stored")
    for name, path in (("A", args.a), ("B", args.b)):
        if path.startswith("synthetic:") or path.lower().endswith(".npy") or os.path.isdir(path):
            ap.error(f"{name} ({path}): .npy, image directories and synthetic: carry RGB; --planes yuv needs a .y4m or raw video (--pix-fmt, --size)")
        if not _is_y4m_file(path) and path != "-" and args.pix_fmt is None:
            ap.error(f"{name} ({path}): --planes yuv needs a .y4m, or raw video with --pix-fmt and --size")
    try:
        check_plane_formats(plane_format(args, args.a), plane_format(args, args.b))
    except ValueError as e:
        ap.error(f"--planes yuv: A and B: {e}")


def _check_ms_ssim(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """--ms-ssim: five scales of RGB frames, on top of the SSIM record."""
    if args.no_ssim:
        ap.error("--ms-ssim builds on the SSIM record that --no-ssim skips: give one of the two")
    if args.planes == "yuv":
        ap.error("--ms-ssim compares RGB frames: --planes yuv is not supported with it")
    size = args.scale if args.scale is not None else args.size  # (W, H) where the command line states it
    if size is None:
        for path in (args.a, args.b):
            if path.startswith("synthetic:"):
                try:
                    size = _size_arg(path.split(":")[1])
                except (IndexError, argparse.ArgumentTypeError):
                    size = None
                break
    if size is not None and (size[0] < MS_MIN_SIDE or size[1] < MS_MIN_SIDE):
        ap.error(f"--ms-ssim: five scales need frames of at least {MS_MIN_SIDE}x{MS_MIN_SIDE}; these are {size[0]}x{size[1]}")


class _CompareParser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        args = super().parse_args(args, namespace)
        for flag, dest in _OUTPUT_ONLY:
            if getattr(args, dest) is not None:
                self.error(f"{flag} belongs to a command that writes video: compare writes none")
        if args.no_ssim and args.min_ssim is not None:
            self.error("--min-ssim needs the SSIM that --no-ssim skips")
        if args.a == "-" and args.b == "-":
            self.error("A and B cannot both be stdin")
        if hasattr(args, "min_ms_ssim"):
            args.ms_ssim = True
        if getattr(args, "ms_ssim", False):
            _check_ms_ssim(self, args)
        if args.planes == "yuv":
            _check_planes_yuv(self, args)
        args.input = args.a  # what check_io_options reads the source size of a synthetic: input from
        check_io_options(self, args)
        check_raw_options(self, args)
        if args.scale is not None and args.size is None and args.b.startswith("synthetic:"):
            try:
                src = _size_arg(args.b.split(":")[1])
            except (IndexError, argparse.ArgumentTypeError):
                src = None
            if src is not None and (args.scale[0] > src[0] or args.scale[1] > src[1]):
                self.error(f"--scale {args.scale[0]}x{args.scale[1]} enlarges the {src[0]}x{src[1]} source: --scale only reduces")
        return args


def build_parser() -> argparse.ArgumentParser:
    ap = _CompareParser(prog="compare", description="PSNR, SSIM and code differences of two videos, frame by frame, on the device.")
    ap.add_argument("a", metavar="A", help=".y4m file, raw video (--pix-fmt), synthetic:<W>x<H>:<n>[:kind], .npy or an image directory")
    ap.add_argument("b", metavar="B", help="the same forms; the input options apply to both")
    add_input_options(ap)
    add_output_options(ap)
    ap.set_defaults(batch=8, depth=None)
    ap.add_argument("--planes", default="rgb", choices=["rgb", "yuv"],
                    help="rgb (default): compare RGB uint8 after decode, tone map and scale.  yuv: compare the Y, U and V planes as stored, at "
                         "8 or 10 bits, in native codes (PSNR-Y/U/V; .y4m or raw video only; a .y4m is I420 whatever --pix-fmt says, so it "
                         "compares against a raw nv12 or yuv420p file); --matrix and --range are accepted and have no effect, --scale and "
                         "--transfer are errors")
    ap.add_argument("--no-ssim", action="store_true", help="histograms (PSNR, max_abs, beyond1) only")
    # both MS-SSIM options leave no attribute behind when they are not given: without them the namespace is what it always was
    ap.add_argument("--ms-ssim", action="store_true", default=argparse.SUPPRESS,
                    help="also MS-SSIM over five scales (columns ms_ssim_r,ms_ssim_g,ms_ssim_b,ms_ssim behind the others); RGB frames of at "
                         "least 176x176 only: --no-ssim and --planes yuv are errors with it")
    ap.add_argument("--csv", default=None, metavar="FILE", help="write the per-frame lines here instead of stdout")
    ap.add_argument("--shortest", action="store_true", help="inputs of different lengths: compare the common prefix without complaint")
    ap.add_argument("--min-psnr", type=float, default=None, metavar="X", help="status 1 when a frame's PSNR (all channels) is below X dB")
    ap.add_argument("--min-ssim", type=float, default=None, metavar="X", help="status 1 when a frame's mean SSIM is below X")
    ap.add_argument("--min-ms-ssim", type=float, default=argparse.SUPPRESS, metavar="X", help="status 1 when a frame's MS-SSIM is below X; implies --ms-ssim")
    ap.add_argument("--max-abs", type=int, default=None, metavar="K", help="status 1 when a frame has samples more than K codes apart")
    ap.add_argument("--max-beyond1", type=float, default=None, metavar="S", help="status 1 when more than the share S of a frame's samples is beyond +-1 code")
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def violation(args, m: FrameMetrics, ms: Optional[MsSsim] = None) -> Optional[str]:
    """What frame record `m` (and, with --ms-ssim, `ms`) violates of the command line's limits, None when nothing."""
    if args.min_psnr is not None and m.psnr < args.min_psnr:
        return f"PSNR {_num(m.psnr)} dB is below --min-psnr {args.min_psnr:g}"
    if args.min_ssim is not None and not m.ssim_mean >= args.min_ssim:
        return f"SSIM {_num(m.ssim_mean)} is below --min-ssim {args.min_ssim:g}"
    if ms is not None and getattr(args, "min_ms_ssim", None) is not None and not ms.ms_ssim >= args.min_ms_ssim:
        return f"MS-SSIM {_num(ms.ms_ssim)} is below --min-ms-ssim {args.min_ms_ssim:g}"
    if args.max_abs is not None and m.max_abs > args.max_abs:
        return f"largest difference {m.max_abs} is above --max-abs {args.max_abs}"
    if args.max_beyond1 is not None and m.share_beyond(1) > args.max_beyond1:
        return f"share beyond +-1 code {m.share_beyond(1):.6g} is above --max-beyond1 {args.max_beyond1:g}"
    return None


# ------------------------------------------------------------------------------------------------ the device loop
def _renderer(args, path: str):
    from .renderers import VideoRenderer

    if getattr(args, "planes", "rgb") == "yuv":
        raw = not _is_y4m_file(path) and args.pix_fmt is not None
        return VideoRenderer(read_path=path, write_path=None, pix_fmt=args.pix_fmt if raw else None, size=args.size if raw else None)
    return VideoRenderer(read_path=path, write_path=None, matrix=args.matrix, range=args.range, pix_fmt=args.pix_fmt, size=args.size,
                         transfer=args.transfer, tonemap=args.tonemap, peak_nits=args.peak_nits, sdr_white=args.sdr_white, scale=args.scale)


def _open(args, path: str):
    """The opened renderer of `path` and the (H, W) of the frames it will be compared at."""
    vr = _renderer(args, path)
    vr.open()
    hw = vr.out_hw
    if hw is None:  # synthetic:, .npy or an image directory: peek at the first frame, then start over
        first = vr.get_image()
        hw = None if first is None else tuple(first.shape[:2])
        vr.close()
        vr = _renderer(args, path)
        vr.open()
    return vr, hw


class _Side:
    """One input: its staging (pinned) and device buffers, one of each per buffer set."""

    def __init__(self, ctx, vr, H: int, W: int, batch: int, sets: int):
        from .yuv import frame_size

        self.ctx, self.vr, self.H, self.W = ctx, vr, H, W
        self.payload = vr.yuv_hw is not None and vr.scale is None and vr.transfer is None
        self.fmt = vr.yuv_pix_fmt  # None: I420 (.y4m)
        self.unit = frame_size(self.fmt or "yuv420p", H, W) if self.payload else H * W * 3
        self.host = [ctx.pinned((batch, self.unit), np.uint8) for _ in range(sets)]
        self.d_rgb = [ctx.malloc(batch * H * W * 3) for _ in range(sets)]
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
                raise SystemExit(f"compare: {self.vr.read_path}: frame {self.vr.last_index} is {f.dtype} {f.shape}, not uint8 {(self.H, self.W, 3)}")
            self.host[k].array[n] = f.reshape(-1)
            n += 1
        return n

    def enqueue(self, k: int, n: int, stream) -> None:
        from ._lib import lib
        from .yuv import i420_to_rgb_device, yuv_to_rgb_device

        ctx = self.ctx
        ctx._check(lib.avx_memcpy_h2d(ctx._h, self.d_in[k].ptr, self.host[k].ptr, n * self.unit, stream))
        if self.payload and self.fmt is None:
            i420_to_rgb_device(ctx, self.d_in[k], self.d_rgb[k], n, self.H, self.W, matrix=self.vr.matrix, range=self.vr.yuv_range, stream=stream)
        elif self.payload:
            yuv_to_rgb_device(ctx, self.fmt, self.d_in[k], self.d_rgb[k], n, self.H, self.W, matrix=self.vr.matrix, range=self.vr.yuv_range,
                              stream=stream)

    def free(self) -> None:
        for b in self.d_rgb + (self.d_in if self.payload else []):
            b.free()
        for h in self.host:
            h.free()


class _PlaneSide:
    """One input of --planes yuv: payloads only, staged (pinned) and uploaded as they are stored; one buffer of each per set."""

    def __init__(self, ctx, vr, H: int, W: int, batch: int, sets: int):
        from .yuv import frame_size

        if vr.yuv_hw is None:
            raise SystemExit(f"compare: {vr.read_path}: --planes yuv needs a .y4m or raw video input")
        self.ctx, self.vr = ctx, vr
        self.fmt = vr.yuv_pix_fmt or "yuv420p"
        self.unit = frame_size(self.fmt, H, W)
        self.host = [ctx.pinned((batch, self.unit), np.uint8) for _ in range(sets)]
        self.d_in = [ctx.malloc(batch * self.unit) for _ in range(sets)]

    def fill(self, k: int, limit: int) -> int:
        n = 0
        while n < limit:
            f = self.vr.get_yuv()
            if f is None:
                break
            self.host[k].array[n] = np.asarray(f).reshape(-1)
            n += 1
        return n

    def enqueue(self, k: int, n: int, stream) -> None:
        from ._lib import lib

        self.ctx._check(lib.avx_memcpy_h2d(self.ctx._h, self.d_in[k].ptr, self.host[k].ptr, n * self.unit, stream))

    def free(self) -> None:
        for b in self.d_in:
            b.free()
        for h in self.host:
            h.free()


def stream_metrics(args, info: dict) -> Iterator[FrameMetrics]:
    """The records of the common prefix of args.a and args.b, in frame order; with --ms-ssim every item is the pair (FrameMetrics,
    MsSsim).  info["longer"] names the input ("A" / "B") that had frames left over, when one had."""
    from ._lib import lib
    from .runtime import get_context

    va, hwa = _open(args, args.a)
    vb, hwb = _open(args, args.b)
    sides = []
    try:
        if hwa is not None and hwb is not None and tuple(hwa) != tuple(hwb):
            raise SystemExit(f"compare: frame sizes differ: A is {hwa[1]}x{hwa[0]}, B is {hwb[1]}x{hwb[0]}")
        if hwa is None or hwb is None:  # an empty input
            if hwa is not None or hwb is not None:
                info["longer"] = "A" if hwa is not None else "B"
            return
        H, W = hwa
        ctx, batch, sets = get_context(), args.batch, 2
        yuv = getattr(args, "planes", "rgb") == "yuv"
        ms = bool(getattr(args, "ms_ssim", False))
        if ms and (H < MS_MIN_SIDE or W < MS_MIN_SIDE):
            raise SystemExit(f"compare: --ms-ssim: five scales need frames of at least {MS_MIN_SIDE}x{MS_MIN_SIDE}; these are {W}x{H}")
        rec_bytes = PLANE_RECORD_BYTES if yuv else RECORD_BYTES
        side = _PlaneSide if yuv else _Side
        sides.append(side(ctx, va, H, W, batch, sets))
        sides.append(side(ctx, vb, H, W, batch, sets))
        streams = [ctx.stream_create() for _ in range(sets)]
        d_out = [ctx.malloc(batch * rec_bytes) for _ in range(sets)]
        h_out = [ctx.pinned((batch * rec_bytes,), np.uint8) for _ in range(sets)]
        d_ms = [ctx.malloc(batch * MS_RECORD_BYTES) for _ in range(sets)] if ms else []
        h_ms = [ctx.pinned((batch * MS_RECORD_BYTES,), np.uint8) for _ in range(sets)] if ms else []
        pending = [0] * sets

        def harvest(k):
            ctx.sync(streams[k])
            n, pending[k] = pending[k], 0
            if yuv:
                return plane_records_from_bytes(h_out[k].array, n, sides[0].fmt, H, W) if n else []
            if ms:
                return list(zip(records_from_bytes(h_out[k].array, n), ms_records_from_bytes(h_ms[k].array, n))) if n else []
            return records_from_bytes(h_out[k].array, n) if n else []

        try:
            i = 0
            while True:
                k = i % sets
                yield from harvest(k)  # the set's previous batch: its buffers are free again afterwards
                na, nb = sides[0].fill(k, batch), sides[1].fill(k, batch)
                n = min(na, nb)
                if n:
                    for s in sides:
                        s.enqueue(k, n, streams[k])
                    if yuv:
                        plane_metrics_launch(ctx, sides[0].fmt, sides[0].d_in[k], sides[1].d_in[k], n, H, W, d_out[k], pix_fmt_b=sides[1].fmt,
                                             ssim=not args.no_ssim, stream=streams[k])
                    elif ms:
                        frame_metrics_ms_launch(ctx, sides[0].d_rgb[k], sides[1].d_rgb[k], n, H, W, d_out[k], d_ms[k], stream=streams[k])
                        ctx._check(lib.avx_memcpy_d2h(ctx._h, h_ms[k].ptr, d_ms[k].ptr, n * MS_RECORD_BYTES, streams[k]))
                    else:
                        frame_metrics_launch(ctx, sides[0].d_rgb[k], sides[1].d_rgb[k], n, H, W, d_out[k], ssim=not args.no_ssim,
                                             stream=streams[k])
                    ctx._check(lib.avx_memcpy_d2h(ctx._h, h_out[k].ptr, d_out[k].ptr, n * rec_bytes, streams[k]))
                    pending[k] = n
                i += 1
                if na != nb:
                    info["longer"] = "A" if na > nb else "B"
                if n < batch:
                    break
            for j in range(sets):
                yield from harvest((i + j) % sets)
        finally:
            for k in range(sets):
                ctx.sync(streams[k])
                ctx.stream_destroy(streams[k])
            for b in d_out + d_ms:
                b.free()
            for h in h_out + h_ms:
                h.free()
    finally:
        for s in sides:
            s.free()
        va.close()
        vb.close()


# ------------------------------------------------------------------------------------------------ the command
def _psnr_peak(sse: int, n: int, peak: int) -> float:
    return math.inf if sse == 0 else 10.0 * math.log10(float(peak) ** 2 * n / sse)


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    yuv, with_ms = args.planes == "yuv", bool(getattr(args, "ms_ssim", False))
    min_ms, sum_ms = math.inf, 0.0
    sse_y = samples_y = 0  # --planes yuv: the luma plane's share of the pooled sums, and the depth the records name
    depth = None
    info: dict = {}
    frames, first_bad, worst_abs, min_ssim, sum_ssim = 0, None, 0, math.inf, 0.0
    sse = samples = beyond = 0
    t0 = time.perf_counter()
    records = stream_metrics(args, info)
    head = list(itertools.islice(records, 1))  # the inputs are opened and their sizes checked before anything is written
    out = open(args.csv, "w") if args.csv else sys.stdout
    try:
        out.write((CSV_HEADER_YUV if yuv else CSV_HEADER) + (CSV_MS_COLUMNS if with_ms else "") + "\n")
        for m in itertools.chain(head, records):
            ms = None
            if with_ms:
                m, ms = m
                sum_ms += ms.ms_ssim
                min_ms = min(min_ms, ms.ms_ssim)
            out.write((format_row_planes(frames, m) if yuv else format_row(frames, m)) + (format_ms_columns(ms) if with_ms else "") + "\n")
            if first_bad is None:
                why = violation(args, m, ms)
                if why is not None:
                    first_bad = (frames, why)
            sse += sum(m.sse)
            if yuv:
                samples += m.samples
                sse_y, samples_y, depth = sse_y + m.sse[0], samples_y + m.plane_samples[0], m.depth
            else:
                samples += 3 * m.samples
            beyond += m.count_beyond(1)
            worst_abs = max(worst_abs, m.max_abs)
            if not args.no_ssim:
                sum_ssim += m.ssim_mean
                min_ssim = min(min_ssim, m.ssim_mean)
            frames += 1
    finally:
        if out is not sys.stdout:
            out.close()
        else:
            out.flush()
    dt = time.perf_counter() - t0
    ssim_txt = "SSIM skipped" if args.no_ssim or not frames else f"SSIM mean {sum_ssim / frames:.6f} min {min_ssim:.6f}"
    if with_ms and frames:
        ssim_txt += f", MS-SSIM mean {sum_ms / frames:.6f} min {min_ms:.6f}"
    if yuv:
        peak = (1 << depth) - 1 if frames else 255
        psnr_txt = (f"PSNR-Y {_num(_psnr_peak(sse_y, samples_y, peak)) if frames else 'nan'} dB, "
                    f"PSNR {_num(_psnr_peak(sse, samples, peak)) if frames else 'nan'} dB ({depth if frames else '?'}-bit)")
    else:
        psnr_txt = f"PSNR {_num(_psnr(sse, samples)) if frames else 'nan'} dB"
    print(f"compare: {frames} frames, {psnr_txt}, {ssim_txt}, largest difference {worst_abs}, "
          f"beyond +-1 code {beyond / samples if samples else 0.0:.6g}, {frames / dt if dt > 0 else 0.0:.1f} fps", file=sys.stderr)
    status = 0
    if info.get("longer") and not args.shortest:
        print(f"compare: {info['longer']} has more frames than the other input: compared the first {frames} (--shortest accepts that)", file=sys.stderr)
        status = 2
    if first_bad is not None:
        print(f"compare: frame {first_bad[0]}: {first_bad[1]}", file=sys.stderr)
        status = 1
    return status


if __name__ == "__main__":
    sys.exit(main())
