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
is written; of different lengths, the common prefix is compared and the status is 2 unless --shortest is given.

--ppd X switches to S-CIELAB (Zhang & Wandell 1996): both frames are first filtered in an opponent colour space by the
eye's contrast sensitivity for a viewer who sees X pixels per degree of visual angle, and dE00 is taken on the filtered frames.  A
per-pixel dE charges resampling, ringing and blur at the pixel scale in full even where nobody could resolve them; with --ppd they
count for what is left of them at that distance.  X = pixels per unit length x viewing distance x tan 1 degree: a 1080-line picture
seen from three picture heights is about 57, and 60 is the usual round number; no default is applied, because the answer depends on
it.  Finite, from 2 to 128.  Everything else keeps its meaning: the columns, the limits, --threshold, the modes, the layouts (the dim
grey and the A and B panels are the unfiltered frames), all sources and sinks.  Without --ppd nothing changes.

    python -m animal_vision_amd.deltae full.y4m half.y4m --ppd 60 --max-p95 2

--observer NAME --weber E1,E2[,E3] [--floor EPS] asks the question of another animal: can a dog, or a bee, tell the two
clips apart, and where in the frame.  The value of a pixel is then the receptor-noise-limited distance dS of Vorobyev & Osorio (1998)
in place of dE00: every receptor class of the observer contributes the logarithm of the ratio of its two catches, weighted by the
noise of the class -- its Weber fraction --, and the result is in just-noticeable differences, so --threshold 1 keeps its meaning.
NAME is one of the 20 dichromats (two classes, in the order LM, S: the species' alpha-weighted L and M, and S) or HoneyBee (three:
UV, Blue, Green); the UV plane-program species, Mantis Shrimp and RatUV have no such matrix on RGB and are refused.  The Weber
fractions are yours, one per class, each from 0.01 to 1: there is no per-species table (for the honeybee 0.13,0.06,0.12 are the values
commonly cited from Vorobyev et al. 2001).  EPS (1e-6 to 0.1, default 0.001) is added to every catch before the logarithm and bounds
what near-black pixels can contribute.  The measure is chromatic: every receptor class is adapted to white, and two greys are 0 apart
whatever their brightness.  It is a per-pixel measure of the frames as given: it does not combine with --ppd.  Everything else keeps
its meaning: the columns, the limits, --threshold, the modes, the layouts, all sources and sinks.  Without --observer nothing changes.

    python -m animal_vision_amd.deltae ripe.y4m unripe.y4m heat.y4m --observer Dog --weber 0.05,0.05 --layout side
    python -m animal_vision_amd.deltae flower.y4m leaf.y4m --observer HoneyBee --weber 0.13,0.06,0.12 --csv bee.csv

--acuity SIGMA|species, with --observer, puts the observer's acuity in front of the distance (AcuityView, Caves & Johnsen
2018, then the receptor distance: the first two stages of QCPA): both frames are blurred in linear light by a Gaussian of SIGMA pixels
before the catches are taken, so that detail the animal cannot resolve -- resampling, fine texture, noise -- counts for what is left of
it.  `species` takes the blur the species' own rendering ends with (Dog 3.5, Cat 1.0, ...: the ten dichromats with a Gaussian acuity;
the others are refused by name, with the reason); a number is in pixels of the frames as compared, after --scale, from 0.2 to 4.
Everything else keeps its meaning; the dim grey and the A and B panels are the unfiltered frames.  Without --acuity nothing changes.

    python -m animal_vision_amd.deltae full.y4m half.y4m --observer Dog --weber 0.05,0.05 --acuity species --max-p95 1

--itp switches to dE_ITP of ITU-R BT.2124: 720 x the distance in ICtCp with Ct halved, about 1 per just-noticeable
difference, and defined at HDR light levels, where dE00 is not.  An input read as raw video with a 10-bit --pix-fmt (and --size) is an
HDR side -- --transfer pq|hlg is then required --: it crosses to the device as its payload and is compared as stored, in display
light, with no tone map in between.  Every other input (.y4m, .npy, an image directory, synthetic:, 8-bit raw video) is an SDR side:
8-bit sRGB, decoded as without --transfer, with code 255 shown at --sdr-white nits (default 203).  So the SDR rendering of an HDR master
can be held against the master itself, or two tone maps, or two encodes of one HDR clip, against each other.  With OUT an HDR side is
also decoded once with --tonemap, --peak-nits and --sdr-white: that is what the dim grey and the A and B panels show.  Everything else
keeps its meaning: the columns, --threshold (1 is about one just-noticeable difference), the modes, the layouts, the limits, all
sinks.  It is a per-pixel measure of the frames as stored: it does not combine with --ppd, --observer, --acuity or --scale.  Without
--itp nothing changes.

    python -m animal_vision_amd.deltae master.yuv sdr.y4m --pix-fmt p010le --size 3840x2160 --transfer pq --itp --max-p95 3"""
from __future__ import annotations

import argparse
import math
import sys
import time
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np

from .metrics import (DELTA_E_DEFAULT_GAIN, DELTA_E_DEFAULT_THRESHOLD, DELTA_E_LAYOUTS, DELTA_E_MODES, DELTA_E_RECORD_BYTES, RECEPTOR_DEFAULT_FLOOR,
                      DeltaE, ItpSide, check_acuity, check_delta_e_options, check_ppd, delta_e_launch, delta_e_records_from_bytes, itp_delta_launch,
                      observer_for, observer_names, receptor_delta_launch, scielab_launch, species_acuity)
from .pairs import (add_inputs, check_depth, check_inputs, check_stdin, exit_status, is_raw_input, num, open_sink, opened,  # noqa: F401
                    sink_format, stream_map_pairs)
from .video import add_input_options, add_output_options

CSV_HEADER = "frame,de_mean,de_p50,de_p95,de_max,x,y,beyond"
_OUTPUT_ONLY = (("--out-pix-fmt", "out_pix_fmt"), ("--out-matrix", "out_matrix"), ("--depth", "depth"), ("--mode", "mode"), ("--gain", "gain"),
                ("--layout", "layout"))


def format_row(index: int, r: DeltaE) -> str:
    """The CSV line of frame `index`."""
    return ",".join([str(index), num(r.mean), num(r.percentile(0.5)), num(r.percentile(0.95)), num(r.max_de), str(r.max_x), str(r.max_y),
                     str(r.beyond)])


def violation(args, r: DeltaE) -> Optional[str]:
    """What record `r` violates of the command line's limits, None when nothing."""
    if args.max_mean is not None and r.mean > args.max_mean:
        return f"mean dE {num(r.mean)} is above --max-mean {args.max_mean:g}"
    if args.max_p95 is not None and r.percentile(0.95) > args.max_p95:
        return f"95th percentile dE {num(r.percentile(0.95))} is above --max-p95 {args.max_p95:g}"
    if args.max_de is not None and r.max_de > args.max_de:
        return f"largest dE {num(r.max_de)} (pixel x {r.max_x} y {r.max_y}) is above --max-de {args.max_de:g}"
    return None


def itp_side_kind(args, path: str) -> str:
    """What `path` is to --itp: "hdr" when it is read as raw video with a 10-bit --pix-fmt, else "sdr"."""
    from .yuv import HDR_PIX_FMTS

    return "hdr" if is_raw_input(args, path) and args.pix_fmt in HDR_PIX_FMTS else "sdr"


def _itp_renderer(args, path: str):
    """The renderer of one input of --itp: an HDR side with the HDR options (its decode makes the panel), every other input as
    without --transfer, and --pix-fmt / --size only where the input is raw video."""
    from .renderers import VideoRenderer

    if itp_side_kind(args, path) == "hdr":
        return VideoRenderer(read_path=path, write_path=None, range=args.range, pix_fmt=args.pix_fmt, size=args.size, transfer=args.transfer,
                             tonemap=args.tonemap, peak_nits=args.peak_nits, sdr_white=args.sdr_white)
    raw = is_raw_input(args, path)
    return VideoRenderer(read_path=path, write_path=None, matrix=args.matrix, range=args.range, pix_fmt=args.pix_fmt if raw else None,
                         size=args.size if raw else None)


class _DeltaEParser(argparse.ArgumentParser):
    def _itp(self, args):
        """The checks of --itp that need no file; the kind of each side is left in args.itp_kinds."""
        for flag, v in (("--ppd", args.ppd), ("--observer", args.observer), ("--acuity", args.acuity), ("--scale", args.scale)):
            if v is not None:
                self.error(f"--itp and {flag} do not combine: dE_ITP is taken per pixel of the frames as stored")
        args.itp_kinds = tuple(itp_side_kind(args, p) for p in (args.a, args.b))
        for path, kind in zip((args.a, args.b), args.itp_kinds):
            if kind == "hdr" and args.transfer is None:
                self.error(f"--itp: {path} is raw {args.pix_fmt} video, an HDR side: --transfer pq|hlg must name its transfer function")

    def _observer(self, args):
        """The metrics.Observer that --observer, --weber and --floor name, or None without them."""
        if args.observer is None:
            for flag, v in (("--weber", args.weber), ("--floor", args.floor)):
                if v is not None:
                    self.error(f"{flag} belongs to --observer NAME: without an observer there are no receptor classes")
            if args.acuity is not None:
                self.error("--acuity belongs to --observer NAME: the acuity is an observer's; dE00 at a viewing distance is --ppd")
            return None
        if args.weber is None:
            self.error("--observer needs --weber E1,E2[,E3]: the Weber fraction of each receptor class; there is no per-species table")
        if args.ppd is not None:
            self.error("--observer and --ppd do not combine: the receptor distance is taken per pixel of the frames as given")
        try:
            weber = [float(v) for v in args.weber.split(",")]
        except ValueError:
            self.error(f"--weber: comma-separated numbers, e.g. 0.05,0.05 (got {args.weber!r})")
        if args.observer not in observer_names():
            self.error(f"--observer: no receptor model on RGB for {args.observer!r}: the observers are {', '.join(observer_names())}")
        try:
            observer = observer_for(args.observer, weber, RECEPTOR_DEFAULT_FLOOR if args.floor is None else args.floor)
        except ValueError as e:
            self.error(f"--weber / --floor: {e}")
        if args.acuity is not None:
            try:
                args.acuity = species_acuity(args.observer) if args.acuity == "species" else check_acuity(self._sigma(args.acuity))
            except ValueError as e:
                self.error(f"--acuity: {e}")
        return observer

    def _sigma(self, text: str) -> float:
        try:
            return float(text)
        except ValueError:
            self.error(f"--acuity: a number of pixels, or `species` for the observer's own (got {text!r})")

    def parse_args(self, args=None, namespace=None):
        args = super().parse_args(args, namespace)
        if args.out is None:
            for flag, dest in _OUTPUT_ONLY:
                if getattr(args, dest) is not None:
                    self.error(f"{flag} shapes the video that OUT names: without OUT deltae writes none")
        check_stdin(self, args)
        args.depth = 2 if args.depth is None else args.depth
        check_depth(self, args)
        args.mode, args.layout = args.mode or "heat", args.layout or "map"
        white = None
        if args.itp:
            self._itp(args)
            if args.transfer is None:  # SDR sides only: --sdr-white is theirs here, and the HDR options' check must not see it
                white, args.sdr_white = args.sdr_white, None
        try:
            args.gain, args.threshold = check_delta_e_options(args.mode, args.gain, args.threshold, args.layout)
        except ValueError as e:
            self.error(f"--gain / --threshold: {e}")
        if args.ppd is not None:
            try:
                args.ppd = check_ppd(args.ppd)
            except ValueError as e:
                self.error(f"--ppd: {e}")
        args.observer = self._observer(args)
        for flag, v in (("--max-mean", args.max_mean), ("--max-p95", args.max_p95), ("--max-de", args.max_de)):
            if v is not None and not (math.isfinite(v) and v >= 0.0):
                self.error(f"{flag} must be finite and at least 0 (got {v:g})")
        check_inputs(self, args)
        if white is not None:
            if not (math.isfinite(white) and white > 0.0):
                self.error(f"--sdr-white must be finite and positive (got {white})")
            args.sdr_white = white
        return args


def build_parser() -> argparse.ArgumentParser:
    ap = _DeltaEParser(prog="deltae", description="CIEDE2000 colour difference of two videos -- or, with --observer, the distance another species' receptors see -- per frame and as a video of "
                                         "maps, computed on the device.")
    add_inputs(ap)
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
    ap.add_argument("--ppd", type=float, default=None, metavar="X",
                    help="S-CIELAB: filter both frames by the eye's contrast sensitivity at X pixels per degree of visual angle before dE is taken "
                         "(X = pixels per unit length x viewing distance x tan 1 degree; a 1080-line picture seen from three picture heights is "
                         "about 57; take 60 when in doubt).  Finite, from 2 to 128.  Default: none, the plain per-pixel dE")
    ap.add_argument("--observer", default=None, metavar="NAME",
                    help="the receptor-noise-limited distance dS (Vorobyev & Osorio 1998), in just-noticeable differences, as this species' receptor "
                         "classes see it, in place of dE: one of the 20 dichromats (two classes: LM, S) or HoneyBee (three: UV, Blue, Green).  "
                         "Needs --weber; chromatic only: two greys are 0 apart.  Default: none, the human dE")
    ap.add_argument("--weber", default=None, metavar="E1,E2[,E3]",
                    help="with --observer: the Weber fraction of each receptor class, in the observer's order, each from 0.01 to 1.  They are "
                         "yours to choose: there is no per-species table (0.13,0.06,0.12 are the values commonly cited for the honeybee from "
                         "Vorobyev et al. 2001)")
    ap.add_argument("--floor", type=float, default=None, metavar="EPS",
                    help=f"with --observer: added to every catch before the logarithm, from 1e-6 to 0.1 (default {RECEPTOR_DEFAULT_FLOOR:g})")
    ap.add_argument("--acuity", default=None, metavar="SIGMA|species",
                    help="with --observer: blur both frames in linear light by the observer's acuity, a Gaussian of SIGMA pixels of the frames as "
                         "compared (0.2 to 4), before the distance is taken.  `species`: the blur the species' own rendering ends with (the ten "
                         "dichromats with a Gaussian acuity, e.g. Dog 3.5).  Default: none, the distance per pixel")
    ap.add_argument("--itp", action="store_true",
                    help="dE_ITP of ITU-R BT.2124 in place of dE00: defined for HDR and SDR light alike.  Raw video read with a 10-bit --pix-fmt is "
                         "an HDR side (needs --transfer) and is compared as stored, without a tone map; every other input is an SDR side with "
                         "code 255 at --sdr-white nits.  Does not combine with --ppd, --observer, --acuity or --scale")
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


# ------------------------------------------------------------------------------------------------ the device loop
def stream_records(args, info: dict, fmt: Optional[str] = None) -> Iterator[Tuple[Optional[np.ndarray], DeltaE]]:
    """(output frame, record) of the common prefix of args.a and args.b, in frame order.  Without args.out the frame is None and no map
    is computed.  Otherwise it is RGB uint8 H x W x 3 (H x 3W x 3 with --layout side) when fmt is None, else the flat payload the
    device encoded it to ("i420", or a raw pixel format name).  info["hw"] is the output frames' (H, W) once the first item is there;
    info["longer"] names the input ("A" / "B") that had frames left over, when one had.  The loop is pairs.stream_map_pairs;
    args.observer and args.ppd pick the launch: receptor_delta_launch with an observer (and args.acuity, when there is one), scielab_launch
    with ppd, else delta_e_launch.  With args.itp the launch is itp_delta_launch on the sides as they are: an HDR side's payloads as
    stored, with its decode as the panel when there is a map."""
    if getattr(args, "itp", False):
        def launch_itp(ctx, sides, k, n, H, W, d_map, d_rec, stream):
            ss = [ItpSide(s.d_in[k], s.fmt, args.transfer, s.vr.yuv_range, s.d_rgb[k] if s.d_rgb else None) if s.hdr else ItpSide(s.d_rgb[k]) for s in sides]
            itp_delta_launch(ctx, ss[0], ss[1], n, H, W, d_map, d_rec, sdr_white=args.sdr_white, mode=args.mode, gain=args.gain,
                             threshold=args.threshold, layout=args.layout, stream=stream)

        return stream_map_pairs(args, info, "deltae", fmt, launch_itp, DELTA_E_RECORD_BYTES, delta_e_records_from_bytes, renderer=_itp_renderer,
                                hdr=[k == "hdr" for k in args.itp_kinds], launch_sides=True)

    def launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, stream):
        kw = dict(mode=args.mode, gain=args.gain, threshold=args.threshold, layout=args.layout, stream=stream)
        if getattr(args, "observer", None) is not None:
            if getattr(args, "acuity", None) is not None:
                kw["acuity"] = args.acuity
            receptor_delta_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, observer=args.observer, **kw)
        elif getattr(args, "ppd", None) is None:
            delta_e_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, **kw)
        else:
            scielab_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, ppd=args.ppd, **kw)

    return stream_map_pairs(args, info, "deltae", fmt, launch, DELTA_E_RECORD_BYTES, delta_e_records_from_bytes)


# ------------------------------------------------------------------------------------------------ the command
def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    fmt = sink_format(args)
    info: dict = {}
    frames = beyond = 0
    sum_mean, first_bad = 0.0, None
    worst = (0.0, 0, 0, 0)  # max_de, frame, x, y
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
    observer = getattr(args, "observer", None)
    acuity = getattr(args, "acuity", None)
    blur = "" if acuity is None else f", acuity {acuity:g} px"
    what = f"RNL dS ({observer.describe()}{blur})" if observer is not None else "dE" if args.ppd is None else f"S-CIELAB dE (ppd {args.ppd:g})"
    if getattr(args, "itp", False):
        what = f"dE_ITP ({args.transfer + ', ' if 'hdr' in args.itp_kinds else ''}sdr white {args.sdr_white:g})"
    unit = "dS" if observer is not None else "dE"
    print(f"deltae: {frames} frames, mean {what} {num(sum_mean / frames) if frames else 'nan'}, largest {unit} {num(worst[0])}{where}, "
          f"{beyond} pixels beyond {args.threshold:g}, {frames / dt if dt > 0 else 0.0:.1f} fps", file=sys.stderr)
    return exit_status("deltae", args, info, frames, first_bad)


if __name__ == "__main__":
    sys.exit(main())
