"""The `deltae` command: how far apart two videos are in perceptual units -- CIEDE2000 (dE00) in CIELAB per pixel, computed on the device
 -- as per-frame statistics and, with OUT, as a video of colour difference maps:

    python -m animal_vision_amd.deltae full.y4m half.y4m --max-p95 2
    python -m animal_vision_amd.deltae human.y4m dog.y4m heat.y4m --layout side --csv de.csv
    python -m animal_vision_amd.deltae a.yuv b.yuv maps/ --pix-fmt nv12 --size 3840x2160 --mode plain --gain 4

`compare` gives PSNR and SSIM and `diff` shows where the codes differ; neither measures colour: a one-code step in blue near black and
one in green at mid grey are the same PSNR and not the same visible difference.  A and B are any two source forms of
renderers.VideoRenderer and the input-side options of `video` apply to both, exactly as in `compare` and `diff`: frames are compared
as 8-bit sRGB, RGB uint8 after decode, tone map and scale.

Without OUT no map is computed: one CSV line per frame goes to stdout, or to --csv FILE, and the options that shape a written video
(--out-pix-fmt, --out-matrix, --depth, --mode, --gain, --layout) are errors.  With OUT -- any sink form of `video`: a .y4m file, "-",
raw video, .npy, or a directory of PNG frames -- one map is written per compared pair, encoded on the device for .y4m and raw sinks,
and the CSV goes only to --csv, because stdout may be the video.  With T = --threshold (default 1, about one just-noticeable
difference) and G = --gain (above 0, at most 255; default 10):
  --mode heat   (the default) where dE <= T the pixel is `diff`'s dim grey of A; elsewhere pal(min(255, floor(G (dE - T) + 0.5))),
                `diff`'s palette: black, red, yellow, white.
  --mode plain  pal(min(255, floor(G dE + 0.5))) everywhere; identical frames give a black map.
--layout side writes A | B | map, three times as wide, from the same kernel launch.

The CSV columns are frame,de_mean,de_p50,de_p95,de_max,x,y,beyond: the mean dE of the frame, the median and the 95th percentile read
off a histogram of 0.5-wide bins (the upper edge of the bin that holds it), the largest dE and the first pixel (raster order) that
attains it, and the number of pixels with dE > T.  --max-mean, --max-p95 and --max-de set limits: status 1, and a line on stderr that
names the first frame that breaks one.  A summary line goes to stderr.  Inputs of different frame sizes are an error before anything
is written; of different lengths, the common prefix is compared and the status is 2 unless --shortest is given."""
from __future__ import annotations

import argparse
import itertools
import math
import sys
import time
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np

from .compare import _num, _open, _Side
from .diff import _out_matrix
from .diff import sink_format as _diff_sink_format
from .metrics import (DELTA_E_DEFAULT_GAIN, DELTA_E_DEFAULT_THRESHOLD, DELTA_E_LAYOUTS, DELTA_E_MODES, DELTA_E_RECORD_BYTES, DeltaE,
                      check_delta_e_options, delta_e_launch, delta_e_records_from_bytes)
from .video import _size_arg, add_input_options, add_output_options, check_io_options, check_raw_options

CSV_HEADER = "frame,de_mean,de_p50,de_p95,de_max,x,y,beyond"
_OUTPUT_ONLY = (("--out-pix-fmt", "out_pix_fmt"), ("--out-matrix", "out_matrix"), ("--depth", "depth"), ("--mode", "mode"), ("--gain", "gain"),
                ("--layout", "layout"))


def format_row(index: int, r: DeltaE) -> str:
    """The CSV line of frame `index`."""
    return ",".join([str(index), _num(r.mean), _num(r.percentile(0.5)), _num(r.percentile(0.95)), _num(r.max_de), str(r.max_x), str(r.max_y),
                     str(r.beyond)])


def violation(args, r: DeltaE) -> Optional[str]:
    """What record `r` violates of the command line's limits, None when nothing."""
    if args.max_mean is not None and r.mean > args.max_mean:
        return f"mean dE {_num(r.mean)} is above --max-mean {args.max_mean:g}"
    if args.max_p95 is not None and r.percentile(0.95) > args.max_p95:
        return f"95th percentile dE {_num(r.percentile(0.95))} is above --max-p95 {args.max_p95:g}"
    if args.max_de is not None and r.max_de > args.max_de:
        return f"largest dE {_num(r.max_de)} (pixel x {r.max_x} y {r.max_y}) is above --max-de {args.max_de:g}"
    return None


class _DeltaEParser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        args = super().parse_args(args, namespace)
        if args.out is None:
            for flag, dest in _OUTPUT_ONLY:
                if getattr(args, dest) is not None:
                    self.error(f"{flag} shapes the video that OUT names: without OUT deltae writes none")
        if args.a == "-" and args.b == "-":
            self.error("A and B cannot both be stdin")
        args.depth = 2 if args.depth is None else args.depth
        if not 1 <= args.depth <= 8:
            self.error(f"--depth must be 1..8 buffer sets (got {args.depth})")
        args.mode, args.layout = args.mode or "heat", args.layout or "map"
        try:
            args.gain, args.threshold = check_delta_e_options(args.mode, args.gain, args.threshold, args.layout)
        except ValueError as e:
            self.error(f"--gain / --threshold: {e}")
        for flag, v in (("--max-mean", args.max_mean), ("--max-p95", args.max_p95), ("--max-de", args.max_de)):
            if v is not None and not (math.isfinite(v) and v >= 0.0):
                self.error(f"{flag} must be finite and at least 0 (got {v:g})")
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
    ap = _DeltaEParser(prog="deltae", description="CIEDE2000 colour difference of two videos, per frame and as a video of maps, computed on the device.")
    ap.add_argument("a", metavar="A", help=".y4m file, raw video (--pix-fmt), synthetic:<W>x<H>:<n>[:kind], .npy or an image directory")
    ap.add_argument("b", metavar="B", help="the same forms; the input options apply to both")
    ap.add_argument("out", metavar="OUT", nargs="?", default=None,
                    help="optional: .y4m file, '-' (stdout: Y4M, or raw video with --pix-fmt / --out-pix-fmt), a raw video file, .npy or a directory "
                         "of PNG frames takes one colour difference map per frame pair.  Without it only the per-frame lines are written")
    add_input_options(ap)
    add_output_options(ap)
    ap.set_defaults(batch=8, depth=None)
    ap.add_argument("--mode", default=None, choices=list(DELTA_E_MODES),
                    help="heat (default): a dim grey of A where dE is within --threshold, a black-red-yellow-white colour of G (dE - T) where it "
                         "is not.  plain: the colour of G dE everywhere")
    ap.add_argument("--gain", type=float, default=None, metavar="G", help=f"above 0 and at most 255 (default {DELTA_E_DEFAULT_GAIN:g})")
    ap.add_argument("--threshold", type=float, default=DELTA_E_DEFAULT_THRESHOLD, metavar="T",
                    help=f"finite, at least 0 (default {DELTA_E_DEFAULT_THRESHOLD:g}, about one just-noticeable difference): heat colours the pixels "
                         "with dE above T; the `beyond` column counts them")
    ap.add_argument("--layout", default=None, choices=list(DELTA_E_LAYOUTS), help="map (default): the map alone.  side: A | B | map, three times as wide")
    ap.add_argument("--csv", default=None, metavar="FILE",
                    help=f"write {CSV_HEADER} per frame here; without OUT the default is stdout, with OUT nothing is written unless this is given")
    ap.add_argument("--shortest", action="store_true", help="inputs of different lengths: compare the common prefix without complaint")
    ap.add_argument("--max-mean", type=float, default=None, metavar="X", help="status 1 when a frame's mean dE is above X")
    ap.add_argument("--max-p95", type=float, default=None, metavar="X", help="status 1 when a frame's 95th percentile dE is above X")
    ap.add_argument("--max-de", type=float, default=None, metavar="X", help="status 1 when a frame has a pixel with dE above X")
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def sink_format(args) -> Optional[str]:
    """What OUT takes, as diff.sink_format names it; None also for no OUT."""
    return None if args.out is None else _diff_sink_format(args)


# ------------------------------------------------------------------------------------------------ the device loop
def stream_records(args, info: dict, fmt: Optional[str] = None) -> Iterator[Tuple[Optional[np.ndarray], DeltaE]]:
    """(output frame, record) of the common prefix of args.a and args.b, in frame order.  Without args.out the frame is None and no map
    is computed.  Otherwise it is RGB uint8 H x W x 3 (H x 3W x 3 with --layout side) when fmt is None, else the flat payload the
    device encoded it to ("i420", or a raw pixel format name).  info["hw"] is the output frames' (H, W) once the first item is there;
    info["longer"] names the input ("A" / "B") that had frames left over, when one had."""
    from ._lib import lib
    from .runtime import get_context
    from .yuv import frame_size, i420_size, rgb_to_i420_device, rgb_to_yuv_device

    va, hwa = _open(args, args.a)
    vb, hwb = _open(args, args.b)
    sides = []
    try:
        if hwa is not None and hwb is not None and tuple(hwa) != tuple(hwb):
            raise SystemExit(f"deltae: frame sizes differ: A is {hwa[1]}x{hwa[0]}, B is {hwb[1]}x{hwb[0]}")
        if hwa is None or hwb is None:  # an empty input
            if hwa is not None or hwb is not None:
                info["longer"] = "A" if hwa is not None else "B"
            return
        H, W = hwa
        with_map = args.out is not None
        Wo = 3 * W if args.layout == "side" else W
        info["hw"] = (H, Wo)
        ctx, batch, sets = get_context(), args.batch, args.depth
        unit = H * Wo * 3 if fmt is None else (i420_size(H, Wo) if fmt == "i420" else frame_size(fmt, H, Wo))
        matrix, yrange = _out_matrix(args), args.range or "limited"
        sides.append(_Side(ctx, va, H, W, batch, sets))
        sides.append(_Side(ctx, vb, H, W, batch, sets))
        streams = [ctx.stream_create() for _ in range(sets)]
        d_map = [ctx.malloc(batch * H * Wo * 3) for _ in range(sets)] if with_map else [None] * sets
        d_pay = [ctx.malloc(batch * unit) for _ in range(sets)] if fmt is not None else d_map
        d_rec = [ctx.malloc(batch * DELTA_E_RECORD_BYTES) for _ in range(sets)]
        h_out = [ctx.pinned((batch, unit), np.uint8) for _ in range(sets)] if with_map else []
        h_rec = [ctx.pinned((batch * DELTA_E_RECORD_BYTES,), np.uint8) for _ in range(sets)]
        pending = [0] * sets

        def harvest(k):
            ctx.sync(streams[k])
            n, pending[k] = pending[k], 0
            recs = delta_e_records_from_bytes(h_rec[k].array, n) if n else []
            if not with_map:
                return [(None, r) for r in recs]
            shape = (H, Wo, 3) if fmt is None else (unit,)
            return [(np.array(h_out[k].array[j]).reshape(shape), recs[j]) for j in range(n)]  # copies: the set is filled again

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
                    delta_e_launch(ctx, sides[0].d_rgb[k], sides[1].d_rgb[k], n, H, W, d_map[k], d_rec[k], mode=args.mode, gain=args.gain,
                                   threshold=args.threshold, layout=args.layout, stream=streams[k])
                    if fmt == "i420":
                        rgb_to_i420_device(ctx, d_map[k], d_pay[k], n, H, Wo, matrix=matrix, range=yrange, stream=streams[k])
                    elif fmt is not None:
                        rgb_to_yuv_device(ctx, fmt, d_map[k], d_pay[k], n, H, Wo, matrix=matrix, range=yrange, stream=streams[k])
                    if with_map:
                        ctx._check(lib.avx_memcpy_d2h(ctx._h, h_out[k].ptr, d_pay[k].ptr, n * unit, streams[k]))
                    ctx._check(lib.avx_memcpy_d2h(ctx._h, h_rec[k].ptr, d_rec[k].ptr, n * DELTA_E_RECORD_BYTES, streams[k]))
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
            for b in d_rec + (d_map if with_map else []) + (d_pay if fmt is not None else []):
                b.free()
            for h in h_out + h_rec:
                h.free()
    finally:
        for s in sides:
            s.free()
        va.close()
        vb.close()


# ------------------------------------------------------------------------------------------------ the command
def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    fmt = sink_format(args)
    info: dict = {}
    frames = beyond = 0
    sum_mean, first_bad = 0.0, None
    worst = (0.0, 0, 0, 0)  # max_de, frame, x, y
    t0 = time.perf_counter()
    items = stream_records(args, info, fmt)
    head = list(itertools.islice(items, 1))  # the inputs are opened and their sizes checked before anything is written
    sink = None
    if args.out is not None:
        from .renderers import VideoRenderer

        sink = VideoRenderer(read_path=None, write_path=args.out, write_pix_fmt=None if fmt in (None, "i420") else fmt, matrix=_out_matrix(args),
                             range=args.range, out_matrix=_out_matrix(args))
        sink.open()
    csv = open(args.csv, "w") if args.csv else (sys.stdout if sink is None else None)
    try:
        if csv:
            csv.write(CSV_HEADER + "\n")
        if sink is not None and fmt is not None and "hw" in info:
            sink.set_output_size(*info["hw"])  # payloads name no size of their own
        for frame, r in itertools.chain(head, items):
            if sink is not None:
                sink.render(frame)
            if csv:
                csv.write(format_row(frames, r) + "\n")
            if first_bad is None:
                why = violation(args, r)
                if why is not None:
                    first_bad = (frames, why)
            if r.max_de > worst[0]:
                worst = (r.max_de, frames, r.max_x, r.max_y)
            sum_mean += r.mean
            beyond += r.beyond
            frames += 1
    finally:
        if sink is not None:
            sink.close()
        if csv is sys.stdout:
            csv.flush()
        elif csv:
            csv.close()
    dt = time.perf_counter() - t0
    where = f" (frame {worst[1]}, pixel x {worst[2]} y {worst[3]})" if worst[0] else ""
    print(f"deltae: {frames} frames, mean dE {_num(sum_mean / frames) if frames else 'nan'}, largest dE {_num(worst[0])}{where}, "
          f"{beyond} pixels beyond {args.threshold:g}, {frames / dt if dt > 0 else 0.0:.1f} fps", file=sys.stderr)
    status = 0
    if info.get("longer") and not args.shortest:
        print(f"deltae: {info['longer']} has more frames than the other input: compared the first {frames} (--shortest accepts that)", file=sys.stderr)
        status = 2
    if first_bad is not None:
        print(f"deltae: frame {first_bad[0]}: {first_bad[1]}", file=sys.stderr)
        status = 1
    return status


if __name__ == "__main__":
    sys.exit(main())
