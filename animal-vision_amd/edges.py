"""The `edges` command: what in a clip stands out to an animal -- per pixel the largest receptor-noise-limited contrast between the pixel
and its neighbours, behind the observer's acuity, computed on the device (Local Edge Intensity Analysis, van den Berg et
al. 2020: the third stage of QCPA, behind the acuity blur and the receptor distance of `deltae --observer --acuity`) -- as per-frame
statistics and, with OUT, as a video of maps:

    python -m animal_vision_amd.edges meadow.y4m --observer Dog --weber 0.05,0.05 --achromatic 1:0.1 --acuity species
    python -m animal_vision_amd.edges flowers.y4m bee.y4m --observer HoneyBee --weber 0.13,0.06,0.12 --achromatic 3:0.12 --channel chromatic
    python -m animal_vision_amd.edges clip.yuv maps/ --pix-fmt nv12 --size 3840x2160 --observer Cat --weber 0.05,0.05 --step 2 --mode plain

`deltae` takes two inputs and says whether the animal can tell them apart; this command takes one and says where the boundaries are
that the animal can see, how strong they are in just-noticeable differences, and -- by --channel -- whether colour or brightness
makes them.  INPUT is any source form of `video` and its input-side options apply; frames are taken as 8-bit sRGB, RGB uint8 after
decode, tone map and scale.

The value of a pixel: the frame is decoded to linear light and, with --acuity, blurred by a Gaussian of SIGMA pixels exactly as
`deltae --acuity` blurs a side (`species`: the blur the observer's own rendering ends with; the observers without a Gaussian acuity are
refused by name).  Every receptor class of --observer NAME (`deltae`'s: the 20 dichromats, two classes LM, S; HoneyBee, three: UV,
Blue, Green) takes its catch, and the logarithm of catch + EPS (--floor, default 0.001) is taken once per pixel.  Between the pixel
and each of its up to eight neighbours D = --step pixels away (1..8; left, right, up, down and the four diagonals; a neighbour
outside the frame is skipped) the chromatic contrast is `deltae --observer`'s distance dS with --weber E1,E2[,E3], and the achromatic
contrast is |difference of the log-catches of the luminance channel| / E, with --achromatic CLASSES:E: CLASSES are the `+`-joined
1-based numbers of the observer's classes whose mean is the luminance channel, E its Weber fraction (0.01 to 1) -- yours to choose, like
the Weber fractions: there is no per-species table (`--observer Dog --achromatic 1:0.1` is the LM class, `--observer HoneyBee
--achromatic 3:0.12` the Green receptor).  --channel chromatic|achromatic|either picks dS, the achromatic contrast or the larger of
the two; the default is either with --achromatic, else chromatic.  The pixel's value is the largest over its neighbours.

--smooth RADIUS:KEEP[:ITERATIONS] puts an edge-preserving smoothing in receptor space in front of the edges, so that
sensor and compression noise, which is exactly a contrast to a neighbour, does not light the map up everywhere: every pixel's
log-catches are averaged with those pixels of the (2 RADIUS + 1)^2 window (RADIUS 1..5) that look alike to the observer -- the
bandwidth is twice the distance to the pixel that ranks at the share KEEP (above 0, at most 1) of the window, and the weights taper to
zero there -- ITERATIONS times (1..8, default 1).  It stands where QCPA has its RNL ranked filter; the definition is this project's own
(micaToolbox's weights could not be pinned), and there is no default for RADIUS or KEEP.  The smoothing uses the channel of the edges,
so with it `either` is no longer the larger of the two single-channel results.

Without OUT no map is computed: one CSV line per frame goes to stdout, or to --csv FILE.  With OUT -- any sink form of `video` -- one
map is written per frame, encoded on the device for .y4m and raw sinks, and the CSV goes only to --csv.  --mode, --gain and --threshold
are `deltae`'s: heat (the default) shows the dim grey of the frame where the value is within T (default 1, one just-noticeable
difference) and the palette colour of G (value - T) elsewhere, plain the colour of G value everywhere.  The CSV columns are `deltae`'s,
frame,de_mean,de_p50,de_p95,de_max,x,y,beyond, of the value.  A summary line goes to stderr.  The command sets no limits and its status
is 0 unless something fails: it measures, it does not check."""
from __future__ import annotations

import argparse
import sys
import time
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np

from .deltae import CSV_HEADER, format_row
from .metrics import (DELTA_E_DEFAULT_GAIN, DELTA_E_DEFAULT_THRESHOLD, DELTA_E_MODES, DELTA_E_RECORD_BYTES, EDGES_CHANNELS, EDGES_MAX_STEP,
                      RECEPTOR_DEFAULT_FLOOR, SMOOTH_MAX_ITERATIONS, SMOOTH_MAX_RADIUS, DeltaE, check_delta_e_options, check_edges_options,
                      delta_e_records_from_bytes, observer_for, observer_names, receptor_edges_launch)
from .pairs import Side, check_depth, copy, named_size, num, open_sink, open_source, opened, out_matrix, sink_format
from .runtime import get_context
from .video import add_input_options, add_output_options, check_io_options, check_raw_options

_OUTPUT_ONLY = (("--out-pix-fmt", "out_pix_fmt"), ("--out-matrix", "out_matrix"), ("--mode", "mode"), ("--gain", "gain"))


class _EdgesParser(argparse.ArgumentParser):
    def _achromatic(self, args, K: int):
        """(classes, weber) of --achromatic CLASSES:E, or None without it."""
        if args.achromatic is None:
            return None
        try:
            names, weber = args.achromatic.split(":")
            classes, weber = tuple(int(v) for v in names.split("+")), float(weber)
        except ValueError:
            self.error(f"--achromatic: CLASSES:E with CLASSES the +-joined class numbers and E the Weber fraction, e.g. 1:0.1 or 1+2:0.05 (got {args.achromatic!r})")
        for k in classes:
            if not 1 <= k <= K:
                self.error(f"--achromatic: class {k} is not one of {args.observer}'s receptor classes 1..{K}")
        return classes, weber

    def _smooth(self, args):
        """(radius, keep, iterations) of --smooth RADIUS:KEEP[:ITERATIONS], or None without it."""
        if args.smooth is None:
            return None
        try:
            parts = args.smooth.split(":")
            if len(parts) not in (2, 3):
                raise ValueError
            radius, keep, iterations = int(parts[0]), float(parts[1]), int(parts[2]) if len(parts) == 3 else 1
        except ValueError:
            self.error(f"--smooth: RADIUS:KEEP[:ITERATIONS] with RADIUS and ITERATIONS whole numbers and KEEP a share of the window, e.g. 3:0.5:2 "
                       f"(got {args.smooth!r})")
        if not 1 <= radius <= SMOOTH_MAX_RADIUS:
            self.error(f"--smooth: RADIUS must be 1..{SMOOTH_MAX_RADIUS} pixels (got {radius})")
        if not 0.0 < keep <= 1.0:  # a nan is neither
            self.error(f"--smooth: KEEP must be above 0 and at most 1 (got {keep:g})")
        if not 1 <= iterations <= SMOOTH_MAX_ITERATIONS:
            self.error(f"--smooth: ITERATIONS must be 1..{SMOOTH_MAX_ITERATIONS} (got {iterations})")
        return radius, keep, iterations

    def parse_args(self, args=None, namespace=None):
        args = super().parse_args(args, namespace)
        if args.out is None:
            for flag, dest in _OUTPUT_ONLY:
                if getattr(args, dest) is not None:
                    self.error(f"{flag} shapes the video that OUT names: without OUT edges writes none")
        check_depth(self, args)
        args.mode = args.mode or "heat"
        try:
            args.gain, args.threshold = check_delta_e_options(args.mode, args.gain, args.threshold, "map")
        except ValueError as e:
            self.error(f"--gain / --threshold: {e}")
        if args.observer is None:
            self.error(f"--observer NAME is required: who looks; the observers are {', '.join(observer_names())}")
        if args.weber is None:
            self.error("--observer needs --weber E1,E2[,E3]: the Weber fraction of each receptor class; there is no per-species table")
        try:
            weber = [float(v) for v in args.weber.split(",")]
        except ValueError:
            self.error(f"--weber: comma-separated numbers, e.g. 0.05,0.05 (got {args.weber!r})")
        if args.observer not in observer_names():
            self.error(f"--observer: no receptor model on RGB for {args.observer!r}: the observers are {', '.join(observer_names())}")
        name = args.observer
        try:
            observer = observer_for(name, weber, RECEPTOR_DEFAULT_FLOOR if args.floor is None else args.floor)
        except ValueError as e:
            self.error(f"--weber / --floor: {e}")
        if args.channel in ("achromatic", "either") and args.achromatic is None:
            self.error(f"--channel {args.channel} needs --achromatic CLASSES:E: without it the observer has no luminance channel")
        if not 1 <= args.step <= EDGES_MAX_STEP:
            self.error(f"--step must be 1..{EDGES_MAX_STEP} pixels (got {args.step})")
        achromatic = self._achromatic(args, observer.n_receptors)
        acuity = args.acuity
        if acuity is not None and acuity != "species":
            try:
                acuity = float(acuity)
            except ValueError:
                self.error(f"--acuity: a number of pixels, or `species` for the observer's own (got {acuity!r})")
        args.channel_given = args.channel is not None
        try:
            _, args.channel, sigma, _ = check_edges_options(observer, achromatic, args.channel, acuity, args.step)
        except ValueError as e:
            self.error(f"--achromatic / --acuity: {e}")
        args.observer, args.achromatic, args.acuity = observer, achromatic, (None if acuity is None else sigma)
        if args.smooth is None:
            del args.smooth  # without --smooth the namespace is what it was
        else:
            args.smooth = self._smooth(args)
        check_io_options(self, args)
        check_raw_options(self, args)
        src = named_size(args, args.input)
        if args.scale is not None and src is not None and (args.scale[0] > src[0] or args.scale[1] > src[1]):
            self.error(f"--scale {args.scale[0]}x{args.scale[1]} enlarges the {src[0]}x{src[1]} source: --scale only reduces")
        return args


def build_parser() -> argparse.ArgumentParser:
    ap = _EdgesParser(prog="edges", description="What stands out to an animal within a video: per pixel the largest receptor-noise-limited contrast to its "
                                                "neighbours, chromatic or achromatic, behind the observer's acuity, per frame and as a video of maps, computed "
                                                "on the device.")
    ap.add_argument("input", metavar="INPUT", help=".y4m file, '-' (stdin), raw video (--pix-fmt), synthetic:<W>x<H>:<n>[:kind], .npy or an image directory")
    ap.add_argument("out", metavar="OUT", nargs="?", default=None,
                    help="optional: .y4m file, '-' (stdout: Y4M, or raw video with --pix-fmt / --out-pix-fmt), a raw video file, .npy or a directory "
                         "of PNG frames takes one map per frame.  Without it only the per-frame lines are written")
    add_input_options(ap)
    add_output_options(ap)
    ap.set_defaults(batch=8, depth=2)
    ap.add_argument("--observer", default=None, metavar="NAME", help="who looks: one of the 20 dichromats (two classes: LM, S) or HoneyBee (three: UV, Blue, Green)")
    ap.add_argument("--weber", default=None, metavar="E1,E2[,E3]",
                    help="the Weber fraction of each receptor class, in the observer's order, each from 0.01 to 1; yours to choose: there is no per-species table")
    ap.add_argument("--floor", type=float, default=None, metavar="EPS",
                    help=f"added to every catch before the logarithm, from 1e-6 to 0.1 (default {RECEPTOR_DEFAULT_FLOOR:g})")
    ap.add_argument("--achromatic", default=None, metavar="CLASSES:E",
                    help="the luminance channel: the +-joined numbers (from 1) of the receptor classes whose mean it is, and its Weber fraction, 0.01 "
                         "to 1 (Dog 1:0.1 is the LM class, HoneyBee 3:0.12 the Green receptor); yours to choose.  Default: none")
    ap.add_argument("--channel", default=None, choices=list(EDGES_CHANNELS),
                    help="the contrast that counts: chromatic (the colour distance dS), achromatic (the luminance channel's) or either (the larger).  "
                         "Default: either with --achromatic, else chromatic")
    ap.add_argument("--acuity", default=None, metavar="SIGMA|species",
                    help="blur the frame in linear light by the observer's acuity, a Gaussian of SIGMA pixels (0.2 to 4), before the contrasts are "
                         "taken.  `species`: the blur the species' own rendering ends with.  Default: none")
    ap.add_argument("--step", type=int, default=1, metavar="D", help=f"the distance to the eight neighbours in pixels, 1..{EDGES_MAX_STEP} (default 1)")
    ap.add_argument("--smooth", default=None, metavar="RADIUS:KEEP[:ITERATIONS]",
                    help=f"smooth the log-catches in front of the edges, keeping the edges: average every pixel with the share KEEP (above 0, at most "
                         f"1) of its (2 RADIUS + 1)^2 window (RADIUS 1..{SMOOTH_MAX_RADIUS}) that looks most like it to the observer, ITERATIONS times "
                         f"(1..{SMOOTH_MAX_ITERATIONS}, default 1).  The project's stand-in for QCPA's RNL ranked filter.  Default: none")
    ap.add_argument("--mode", default=None, choices=list(DELTA_E_MODES),
                    help="heat (default): a dim grey of the frame where the value is within --threshold, a black-red-yellow-white colour of "
                         "G (value - T) where it is not.  plain: the colour of G value everywhere")
    ap.add_argument("--gain", type=float, default=None, metavar="G", help=f"above 0 and at most 255 (default {DELTA_E_DEFAULT_GAIN:g})")
    ap.add_argument("--threshold", type=float, default=DELTA_E_DEFAULT_THRESHOLD, metavar="T",
                    help=f"finite, at least 0 (default {DELTA_E_DEFAULT_THRESHOLD:g}, one just-noticeable difference): heat colours the pixels above T; the "
                         "`beyond` column counts them")
    ap.add_argument("--csv", default=None, metavar="FILE",
                    help=f"write {CSV_HEADER} per frame here; without OUT the default is stdout, with OUT nothing is written unless this is given")
    return ap


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def describe(args) -> str:
    """"Dog, weber 0.05,0.05, floor 0.001, achromatic 1:0.1, channel either, acuity 3.5 px, step 1": the parts that were not given are
    left out."""
    parts = [args.observer.describe()]
    if args.achromatic is not None:
        parts.append(f"achromatic {'+'.join(str(k) for k in args.achromatic[0])}:{args.achromatic[1]:g}")
    if args.channel_given:
        parts.append(f"channel {args.channel}")
    if args.acuity is not None:
        parts.append(f"acuity {args.acuity:g} px")
    smooth = getattr(args, "smooth", None)
    if smooth is not None:
        parts.append(f"smooth {smooth[0]}:{smooth[1]:g}x{smooth[2]}")
    parts.append(f"step {args.step}")
    return ", ".join(parts)


# ------------------------------------------------------------------------------------------------ the device loop
def stream_records(args, info: dict, fmt: Optional[str] = None) -> Iterator[Tuple[Optional[np.ndarray], DeltaE]]:
    """(output frame, record) of every frame of args.input, in order: pairs.stream_pairs' loop with one side.  args.depth buffer sets,
    each with a stream of its own, alternate: the upload of batch i + 1 overlaps the kernels of batch i.  Without args.out the frame is
    None and no map is computed.  Otherwise it is RGB uint8 H x W x 3 when fmt is None, else the flat payload the device encoded the map
    to ("i420", or a raw pixel format name).  info["hw"] is the frames' (H, W) once the first item is there.  Buffers and streams are
    released however the generator ends."""
    from .yuv import Encode

    vr, hw = open_source(args, args.input)
    ctx, side, streams, bufs = None, None, [], []
    try:
        if hw is None:  # an empty input
            return
        H, W = hw
        info["hw"] = (H, W)
        with_map = args.out is not None
        encode = None if fmt is None else Encode(None if fmt == "i420" else fmt, out_matrix(args), args.range or "limited")
        unit = H * W * 3 if fmt is None else encode.frame_bytes(H, W)
        # the map (downloaded as it is where the sink takes RGB), the payload it is encoded to, the records
        outputs = ([(H * W * 3, fmt is None)] if with_map else []) + ([(unit, True)] if fmt is not None else []) + [(DELTA_E_RECORD_BYTES, True)]
        ctx, batch, sets = get_context(), args.batch, args.depth
        side = Side(ctx, vr, H, W, batch, sets, "edges")
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
            if not n:
                return []
            recs = delta_e_records_from_bytes(h_out[k][-1].array, n)
            if not with_map:
                return [(None, r) for r in recs]
            shape = (H, W, 3) if fmt is None else (unit,)
            return [(np.array(h_out[k][-2].array[j]).reshape(shape), recs[j]) for j in range(n)]  # copies: the set is filled again

        i = 0
        while True:
            k = i % sets
            yield from collect(k)  # the set's previous batch: its buffers are free again afterwards
            n = side.fill(k, batch)
            if n:
                side.enqueue(k, n, streams[k])
                receptor_edges_launch(ctx, side.d_rgb[k], n, H, W, d_out[k][0] if with_map else None, d_out[k][-1], observer=args.observer,
                                      achromatic=args.achromatic, channel=args.channel, acuity=args.acuity, step=args.step, mode=args.mode,
                                      gain=args.gain, threshold=args.threshold, stream=streams[k], smooth=getattr(args, "smooth", None))
                if encode is not None:
                    encode.launch(ctx, d_out[k][0], d_out[k][1], n, H, W, streams[k])
                for (nbytes, _), d, h in zip(outputs, d_out[k], h_out[k]):
                    if h is not None:
                        copy(ctx, "d2h", h, d, n * nbytes, streams[k])
                pending[k] = n
            i += 1
            if n < batch:
                break
        for j in range(sets):
            yield from collect((i + j) % sets)
    finally:
        for s in streams:
            ctx.sync(s)
            ctx.stream_destroy(s)
        for b in bufs + ([side] if side is not None else []):
            b.free()
        vr.close()


# ------------------------------------------------------------------------------------------------ the command
def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    fmt = sink_format(args)
    info: dict = {}
    frames = beyond = 0
    sum_mean = 0.0
    worst = (0.0, 0, 0, 0)  # the largest value, frame, x, y
    t0 = time.perf_counter()
    items = opened(stream_records(args, info, fmt))
    sink = open_sink(args, fmt, info) if args.out is not None else None
    csv = open(args.csv, "w") if args.csv else (sys.stdout if sink is None else None)
    try:
        if csv:
            csv.write(CSV_HEADER + "\n")
        for frame, r in items:
            if sink is not None:
                sink.render(frame)
            if csv:
                csv.write(format_row(frames, r) + "\n")
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
    print(f"edges: {frames} frames, mean RNL edges ({describe(args)}) {num(sum_mean / frames) if frames else 'nan'}, largest {num(worst[0])}{where}, "
          f"{beyond} pixels beyond {args.threshold:g}, {frames / dt if dt > 0 else 0.0:.1f} fps", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
