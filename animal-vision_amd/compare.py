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
import math
import os
import sys
import time
from typing import Iterator, Optional, Sequence

from .metrics import (MS_MIN_SIDE, MS_RECORD_BYTES, PLANE_RECORD_BYTES, RECORD_BYTES, FrameMetrics, MsSsim, PlaneMetrics, _psnr,
                      check_plane_formats, frame_metrics_launch, frame_metrics_ms_launch, ms_records_from_bytes, plane_metrics_launch,
                      plane_records_from_bytes, records_from_bytes)
from .pairs import add_inputs, check_inputs, check_stdin, exit_status, named_size, num, opened, stream_pairs
from .video import add_input_options, add_output_options

CSV_HEADER = "frame,psnr_r,psnr_g,psnr_b,psnr,ssim_r,ssim_g,ssim_b,ssim,max_abs,beyond1"
CSV_HEADER_YUV = "frame,psnr_y,psnr_u,psnr_v,psnr,ssim_y,ssim_u,ssim_v,ssim,max_abs,beyond1"
CSV_MS_COLUMNS = ",ms_ssim_r,ms_ssim_g,ms_ssim_b,ms_ssim"  # --ms-ssim: behind CSV_HEADER
_OUTPUT_ONLY = (("--out-pix-fmt", "out_pix_fmt"), ("--out-matrix", "out_matrix"), ("--depth", "depth"))


def format_row(index: int, m: FrameMetrics) -> str:
    """The CSV line of frame `index`."""
    p = m.psnr_channels
    return ",".join([str(index), num(p[0]), num(p[1]), num(p[2]), num(m.psnr), num(m.ssim[0]), num(m.ssim[1]), num(m.ssim[2]),
                     num(m.ssim_mean), str(m.max_abs), f"{m.share_beyond(1):.6g}"])


def format_row_planes(index: int, m: PlaneMetrics) -> str:
    """The CSV line of frame `index` with --planes yuv."""
    p = m.psnr_planes
    return ",".join([str(index), num(p[0]), num(p[1]), num(p[2]), num(m.psnr), num(m.ssim[0]), num(m.ssim[1]), num(m.ssim[2]),
                     num(m.ssim_mean), str(m.max_abs), f"{m.share_beyond(1):.6g}"])


def format_ms_columns(ms: MsSsim) -> str:
    """What --ms-ssim appends to the CSV line of a frame."""
    c = ms.ms_ssim_channels
    return "," + ",".join([num(c[0]), num(c[1]), num(c[2]), num(ms.ms_ssim)])


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
    # (W, H) where the command line states it: --scale, --size, or the first synthetic: input
    size = args.scale or named_size(args, args.a if args.a.startswith("synthetic:") else args.b)
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
        check_stdin(self, args)
        if hasattr(args, "min_ms_ssim"):
            args.ms_ssim = True
        if getattr(args, "ms_ssim", False):
            _check_ms_ssim(self, args)
        if args.planes == "yuv":
            _check_planes_yuv(self, args)
        check_inputs(self, args)
        return args


def build_parser() -> argparse.ArgumentParser:
    ap = _CompareParser(prog="compare", description="PSNR, SSIM and code differences of two videos, frame by frame, on the device.")
    add_inputs(ap)
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
        return f"PSNR {num(m.psnr)} dB is below --min-psnr {args.min_psnr:g}"
    if args.min_ssim is not None and not m.ssim_mean >= args.min_ssim:
        return f"SSIM {num(m.ssim_mean)} is below --min-ssim {args.min_ssim:g}"
    if ms is not None and getattr(args, "min_ms_ssim", None) is not None and not ms.ms_ssim >= args.min_ms_ssim:
        return f"MS-SSIM {num(ms.ms_ssim)} is below --min-ms-ssim {args.min_ms_ssim:g}"
    if args.max_abs is not None and m.max_abs > args.max_abs:
        return f"largest difference {m.max_abs} is above --max-abs {args.max_abs}"
    if args.max_beyond1 is not None and m.share_beyond(1) > args.max_beyond1:
        return f"share beyond +-1 code {m.share_beyond(1):.6g} is above --max-beyond1 {args.max_beyond1:g}"
    return None


# ------------------------------------------------------------------------------------------------ the device loop
def stream_metrics(args, info: dict) -> Iterator[FrameMetrics]:
    """The records of the common prefix of args.a and args.b, in frame order; with --ms-ssim every item is the pair (FrameMetrics,
    MsSsim).  info["longer"] names the input ("A" / "B") that had frames left over, when one had.  The loop is pairs.stream_pairs."""
    yuv = getattr(args, "planes", "rgb") == "yuv"
    ms = bool(getattr(args, "ms_ssim", False))

    def prepare(H, W):
        if ms and (H < MS_MIN_SIDE or W < MS_MIN_SIDE):
            raise SystemExit(f"compare: --ms-ssim: five scales need frames of at least {MS_MIN_SIDE}x{MS_MIN_SIDE}; these are {W}x{H}")

        def enqueue(k, n, stream, sides, outs):
            a, b = sides
            if yuv:
                plane_metrics_launch(a.ctx, a.fmt, a.d_in[k], b.d_in[k], n, H, W, outs[0], pix_fmt_b=b.fmt, ssim=not args.no_ssim, stream=stream)
            elif ms:
                frame_metrics_ms_launch(a.ctx, a.d_rgb[k], b.d_rgb[k], n, H, W, outs[0], outs[1], stream=stream)
            else:
                frame_metrics_launch(a.ctx, a.d_rgb[k], b.d_rgb[k], n, H, W, outs[0], ssim=not args.no_ssim, stream=stream)

        def harvest(n, arrays):
            if yuv:
                return plane_records_from_bytes(arrays[0], n, plane_format(args, args.a), H, W)
            if ms:
                return list(zip(records_from_bytes(arrays[0], n), ms_records_from_bytes(arrays[1], n)))
            return records_from_bytes(arrays[0], n)

        return [(PLANE_RECORD_BYTES if yuv else RECORD_BYTES, True)] + ([(MS_RECORD_BYTES, True)] if ms else []), enqueue, harvest

    return stream_pairs(args, info, "compare", prepare, stored=yuv)


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
    records = opened(stream_metrics(args, info))
    out = open(args.csv, "w") if args.csv else sys.stdout
    try:
        out.write((CSV_HEADER_YUV if yuv else CSV_HEADER) + (CSV_MS_COLUMNS if with_ms else "") + "\n")
        for m in records:
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
        psnr_txt = (f"PSNR-Y {num(_psnr_peak(sse_y, samples_y, peak)) if frames else 'nan'} dB, "
                    f"PSNR {num(_psnr_peak(sse, samples, peak)) if frames else 'nan'} dB ({depth if frames else '?'}-bit)")
    else:
        psnr_txt = f"PSNR {num(_psnr(sse, samples)) if frames else 'nan'} dB"
    print(f"compare: {frames} frames, {psnr_txt}, {ssim_txt}, largest difference {worst_abs}, "
          f"beyond +-1 code {beyond / samples if samples else 0.0:.6g}, {frames / dt if dt > 0 else 0.0:.1f} fps", file=sys.stderr)
    return exit_status("compare", args, info, frames, first_bad)


if __name__ == "__main__":
    sys.exit(main())
