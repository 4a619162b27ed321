"""The `diff` command: where two videos differ, as a video of per-pixel difference maps computed on the device:

    python -m animal_vision_amd.diff full.y4m half.y4m heat.y4m
    python -m animal_vision_amd.diff a.yuv b.yuv maps/ --pix-fmt nv12 --size 3840x2160 --mode ssim --layout side --csv where.csv
    python -m animal_vision_amd.diff a.npy b.npy - --mode abs --gain 64 --out-pix-fmt nv12 | ffplay -f rawvideo -pixel_format nv12 ...

`compare` puts a number on the difference of two renderings; `diff` shows where it lies: along edges, on chroma block boundaries,
on the seam of a scaled decode, or on the 32- or 64-pixel lattice of a tile kernel.  A and B are any two source forms of
renderers.VideoRenderer and the input-side options of `video` apply to both, exactly as in `compare`: frames are compared as a
species would see them, RGB uint8 after decode, tone map and scale.  OUT is any sink form of `video`: a .y4m file, "-" (stdout: Y4M,
or raw video with --pix-fmt / --out-pix-fmt), raw video, .npy, or a directory of PNG frames.  One output frame per compared pair.

With d_c = |a_c - b_c| per channel and d = max_c d_c of a pixel:
  --mode abs   out_c = min(255, G d_c); G = --gain, an integer 1..255 (default 32).
  --mode heat  (the default) the project's contract -- "+-1 code" -- as a picture.  K = --threshold (0..254, default 1).  Where d <= K
               the pixel is a dim grey of A, ((77 r + 150 g + 29 b + 128) >> 8) >> 2; where d > K it is pal(min(255, G (d - K))),
               pal(v) = (min(255, 3v), clamp(3v - 255, 0, 255), clamp(3v - 510, 0, 255)): black, red, yellow, white.
  --mode ssim  the local SSIM of `compare` (11 x 11 Gaussian window, sigma 1.5): pixel (y, x) shows the window centred on it, the
               5-pixel border the nearest window; pal(clamp(floor(255 G (1 - mean of the channels' SSIM) + 0.5), 0, 255)), G = --gain, a
               number above 0 and at most 16 (default 4).  Frames of at least 11 x 11.
--layout side writes A | B | map, three times as wide, from the same kernel launch.

--csv FILE takes frame,max_d,x,y,beyond per frame: the largest d, the first pixel (raster order) that attains it, and the number of
PIXELS with d > K (`compare`'s beyond1 counts samples).  It never goes to stdout, which may be the video.  A summary line goes to
stderr.  Inputs of different frame sizes are an error before any frame is compared; of different lengths, the common prefix is
compared and the status is 2 unless --shortest is given.

--depth buffer sets (1..8, default 2), each with a stream of its own, alternate: the upload of batch i + 1 overlaps the kernels of batch
i.  For .y4m and raw sinks the maps are encoded on the device and the payload is what crosses PCIe; .npy and PNG sinks take RGB."""
from __future__ import annotations

import argparse
import sys
import time
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np

from .metrics import (DIFF_DEFAULT_GAIN, DIFF_LAYOUTS, DIFF_MODES, DIFF_RECORD_BYTES, SSIM_WINDOW, DiffRecord, check_diff_options,
                      diff_map_launch, diff_records_from_bytes)
from .pairs import (add_inputs, check_depth, check_inputs, check_stdin, exit_status, named_size, open_sink, opened, sink_format,  # noqa: F401
                    stream_map_pairs)
from .video import add_input_options, add_output_options

CSV_HEADER = "frame,max_d,x,y,beyond"


def format_row(index: int, r: DiffRecord) -> str:
    """The CSV line of frame `index`."""
    return f"{index},{r.max_d},{r.max_x},{r.max_y},{r.beyond}"


class _DiffParser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        args = super().parse_args(args, namespace)
        check_stdin(self, args)
        check_depth(self, args)
        if args.mode != "ssim" and args.gain is not None and not args.gain.is_integer():
            self.error(f"--gain {args.gain:g}: --mode {args.mode} multiplies code differences and takes an integer 1..255")
        try:
            args.gain = check_diff_options(args.mode, args.gain, args.threshold, args.layout)
        except ValueError as e:
            self.error(f"--gain / --threshold: {e}")
        check_inputs(self, args)
        for path in (args.a, args.b):
            size = args.scale if args.scale is not None else named_size(args, path)
            if args.mode == "ssim" and size is not None and (size[0] < SSIM_WINDOW or size[1] < SSIM_WINDOW):
                self.error(f"--mode ssim needs frames of at least {SSIM_WINDOW}x{SSIM_WINDOW}; these are {size[0]}x{size[1]}")
        return args


def build_parser() -> argparse.ArgumentParser:
    ap = _DiffParser(prog="diff", description="Where two videos differ: a video of per-pixel difference or SSIM maps, computed on the device.")
    add_inputs(ap)
    ap.add_argument("out", metavar="OUT", help=".y4m file, '-' (stdout: Y4M, or raw video with --pix-fmt / --out-pix-fmt), a raw video file, .npy "
                                               "or a directory of PNG frames")
    add_input_options(ap)
    add_output_options(ap)
    ap.set_defaults(batch=8, depth=2)
    ap.add_argument("--mode", default="heat", choices=list(DIFF_MODES),
                    help="abs: min(255, G |a - b|) per channel.  heat (default): a dim grey of A where the pixel is within --threshold, a "
                         "black-red-yellow-white colour of G (d - K) where it is not.  ssim: the local SSIM of `compare`, as 255 G (1 - SSIM)")
    ap.add_argument("--gain", type=float, default=None, metavar="G",
                    help=f"abs and heat: an integer 1..255 (default {DIFF_DEFAULT_GAIN['heat']}); ssim: above 0 and at most 16 (default "
                         f"{DIFF_DEFAULT_GAIN['ssim']:g})")
    ap.add_argument("--threshold", type=int, default=1, metavar="K",
                    help="0..254 (default 1): heat colours the pixels whose largest channel difference is above K; every mode counts them "
                         "(the `beyond` column: pixels, where compare's beyond1 counts samples)")
    ap.add_argument("--layout", default="map", choices=list(DIFF_LAYOUTS), help="map (default): the map alone.  side: A | B | map, three times as wide")
    ap.add_argument("--csv", default=None, metavar="FILE", help="write frame,max_d,x,y,beyond per frame here (never to stdout)")
    ap.add_argument("--shortest", action="store_true", help="inputs of different lengths: compare the common prefix without complaint")
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


# ------------------------------------------------------------------------------------------------ the device loop
def stream_maps(args, info: dict, fmt: Optional[str] = None) -> Iterator[Tuple[np.ndarray, DiffRecord]]:
    """(output frame, record) of the common prefix of args.a and args.b, in frame order.  The frame is RGB uint8 H x W x 3 (H x 3W x 3
    with --layout side) when fmt is None, else the flat payload the device encoded it to ("i420", or a raw pixel format name).
    info["hw"] is the output frames' (H, W) once the first item is there; info["longer"] names the input ("A" / "B") that had frames
    left over, when one had.  The loop is pairs.stream_map_pairs."""
    def check_size(H, W):
        if args.mode == "ssim" and (H < SSIM_WINDOW or W < SSIM_WINDOW):
            raise SystemExit(f"diff: --mode ssim needs frames of at least {SSIM_WINDOW}x{SSIM_WINDOW}; these are {W}x{H}")

    def launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, stream):
        diff_map_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, mode=args.mode, gain=args.gain, threshold=args.threshold, layout=args.layout,
                        stream=stream)

    return stream_map_pairs(args, info, "diff", fmt, launch, DIFF_RECORD_BYTES, diff_records_from_bytes, check_size)


# ------------------------------------------------------------------------------------------------ the command
def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    fmt = sink_format(args)
    info: dict = {}
    frames = beyond = 0
    worst = (0, 0, 0, 0)  # max_d, frame, x, y
    t0 = time.perf_counter()
    items = opened(stream_maps(args, info, fmt))
    sink = open_sink(args, fmt, info)
    csv = open(args.csv, "w") if args.csv else None
    try:
        if csv:
            csv.write(CSV_HEADER + "\n")
        for frame, r in items:
            sink.render(frame)
            if csv:
                csv.write(format_row(frames, r) + "\n")
            if r.max_d > worst[0]:
                worst = (r.max_d, frames, r.max_x, r.max_y)
            beyond += r.beyond
            frames += 1
    finally:
        sink.close()
        if csv:
            csv.close()
    dt = time.perf_counter() - t0
    where = f" (frame {worst[1]}, pixel x {worst[2]} y {worst[3]})" if worst[0] else ""
    print(f"diff: {frames} frames, largest difference {worst[0]}{where}, {beyond} pixels beyond {args.threshold}, "
          f"{frames / dt if dt > 0 else 0.0:.1f} fps", file=sys.stderr)
    return exit_status("diff", args, info, frames)


if __name__ == "__main__":
    sys.exit(main())
