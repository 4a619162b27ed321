"""The reference's `video` command (main.py:53-72): every frame of a video through one species, written as a video --
non-interactive, and with Y4M in and out, so real footage can come and go through ffmpeg:

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m animal_vision_amd.video - out.y4m --species Dog --split-compare

Raw (headerless) video, what `ffmpeg -f rawvideo` and hardware decoders write, is named by `--pix-fmt` and `--size`:

    ffmpeg -i in.mkv -f rawvideo -pix_fmt p010le - | python -m animal_vision_amd.video - out.yuv --species Dog --pix-fmt p010le --size 3840x2160

HDR footage (10-bit BT.2020 with a PQ or HLG transfer: HDR10, HLG broadcasts) is named by `--transfer`; it is tone-mapped to SDR on
the device as it is decoded (`--tonemap`, `--peak-nits`, `--sdr-white`), and the output is SDR in `--out-matrix`:

    ffmpeg -i hdr.mkv -f rawvideo -pix_fmt p010le - | python -m animal_vision_amd.video - out.yuv --species Dog --pix-fmt p010le --size 3840x2160 --transfer pq

`--scale WxH` reduces the frames on the device as they are decoded (cv2's INTER_AREA, never enlarging), so that no
`-vf scale` pass on the CPU is needed and 4K decoder output can run at 1080p; the species and the output have the scaled size:

    ffmpeg -i in.mkv -f rawvideo -pix_fmt nv12 - | python -m animal_vision_amd.video - out.yuv --species HoneyBee --pix-fmt nv12 --size 3840x2160 --scale 1920x1080

With `--transfer` as well (4K HDR10 or HLG run at 1080p: `--pix-fmt p010le --transfer pq --scale 1920x1080`) the HDR decode and the
reduction are one launch per batch too, and no 4K RGB frame is ever written.

`--hsi-model seeded|PATH` (HoneyBee only) takes the 31-band cube from the MST++ network instead of the analytic lobes;
`--hsi-scale S` (HoneyBee only, 0.05 <= S < 1) runs that conversion on the frame reduced by S and enlarges the three cone catches back
(HoneyBee(hsi_downsample=True, hsi_scale=S); with the network: DESIGN §4.12).  No checkpoint ships with the package: PATH is a local
.pth of the reference's MST++ training code, and `seeded` (random weights from a fixed seed) is for testing:

    python -m animal_vision_amd.video in.y4m out.y4m --species HoneyBee --hsi-model mst_plus_plus.pth --hsi-scale 0.5

`--out-pix-fmt` names the output's format; it defaults to the input's when OUTPUT is "-" or ends in .yuv.  Raw in and raw out in one
format keep the payload (1.5 B/px for nv12, 3 B/px for p010le) across the host and PCIe (FramePipeline io_format="yuv").

INPUT and OUTPUT are a .y4m file, "-" (stdin / stdout, Y4M), or the other forms renderers.VideoRenderer takes (synthetic:,
.npy, an image directory).  Species are the display names of gallery.py's registry.  Routing:
  * the dichromats (DichromatOp; Cat and --fov: WideStreamOp, the fused wide-view kernels of DESIGN §4.14 and §4.24), HoneyBee (HoneybeeOp; with
    --hsi-model: ml.MstHoneybeeStreamOp) and the plane-program UV
    species with a fixed plan (SpeciesStreamOp) stream through pipeline.run_video: `--depth` frames in flight, split-compose and labels on the device
    (against each species' own baseline, as visualize() returns it: the plane-program species' is their panorama-warped
    input, Cat's the centre-zoomed input), and, from a .y4m to a .y4m, I420 across the host and PCIe (FramePipeline io_format="i420");
  * every other species (MantisShrimp; RatUV, whose plan depends on the frame; HoneyBee
    with --hsi-scale and no --hsi-model) runs
    visualize() per frame, and the split frame is composed from visualize's own (baseline, out) pair, as the reference does.

`--batch N` (1..16) puts N frames into every pipeline slot: the plane-program species then run their launch chain once per N
frames (planevm.DeviceBackend(frames=N): the frame is a grid dimension of the kernels), the dichromats and HoneyBee hand their
kernels n_frames = N (with --hsi-model the network still runs frame by frame on the slot's stream; Cat's zoom and wide-view
launches take the N frames of a slot each).  The species of the per-frame loop have no batched form: for them `--batch` above 1 is an error.

`--night` shows one of the 20 dichromats by night: the reference's rod vision in front of the species' colour stage, and
with `--bloom S` (0 < S <= 1) its tapetum bloom behind the post stage.  The species streams as by day:

    python -m animal_vision_amd.video in.y4m out.y4m --species Cat --night --bloom 0.12 --split-compare

`--night-auto` decides day or night for every frame: a frame whose median Rec.709 luma is below `--night-threshold T`
(default 0.12, the rule of the reference's RatUV) gets the night view, with `--bloom S` the bloom as well; every other frame the day
view.  The rule has no memory, so a frame's output does not depend on --batch, --depth or the shard -- and a clip that hovers at
the threshold flickers between the two views.  A line on stderr reports how many frames were night.

`--fov PHI:OVERLAP` shows one of the 20 dichromats with the reference's binocular wide view in front of its colour stage (DESIGN
§4.24): each eye sees PHI degrees to either side of its axis, the fields share OVERLAP degrees, the output spans 4 PHI - OVERLAP
degrees of which the camera supplies `--camera-hfov` (default 100); columns no eye finds in the camera's frame are black.  The
split frame's left half is the input zoomed to the human's share of that field (`--fov-ratio`, default 1.30).  It streams like Cat,
with --batch, --night, --night-auto and the rest:

    python -m animal_vision_amd.video in.y4m out.y4m --species Horse --fov 105:40 --split-compare"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time
from typing import Optional, Sequence

import numpy as np

from ._lib import AVX_PIX_FMTS, AVX_TONEMAPS, AVX_TRANSFERS
from .gallery import _CLASS_NAMES, ensure_rgb_uint8, species_class

SPECIES_NAMES = list(_CLASS_NAMES)  # all 36 display names


def make_animal(args):
    """The species the parsed command line names, configured by its flags (--hsi-model, --hsi-scale: HoneyBee)."""
    cls = species_class(args.species)
    kw = {}
    if getattr(args, "hsi_scale", None) is not None:
        kw.update(hsi_downsample=True, hsi_scale=args.hsi_scale)
    if getattr(args, "hsi_model", None) is not None:
        from .ml import MSTPlusPlusPredictor

        kw["hsi_model"] = MSTPlusPlusPredictor(None if args.hsi_model == "seeded" else args.hsi_model, seed=0, half=True)
    if getattr(args, "night", False) or getattr(args, "night_auto", False):
        from .dichromat import NIGHT_THRESHOLD, AutoNight, NightSpec

        kw["night"] = NightSpec(bloom=args.bloom if getattr(args, "bloom", None) is not None else 0.0)
        if getattr(args, "night_auto", False):
            thr = getattr(args, "night_threshold", None)
            kw["night"] = AutoNight(kw["night"], NIGHT_THRESHOLD if thr is None else thr)
    if getattr(args, "fov", None) is not None:
        from .dichromat import FovSpec

        cam, ratio = getattr(args, "camera_hfov", None), getattr(args, "fov_ratio", None)
        kw["fov"] = FovSpec(args.fov[0], args.fov[1], 100.0 if cam is None else cam, 1.30 if ratio is None else ratio)
    return cls(**kw)


def route(animal) -> str:
    """The kind of `animal`'s frame operator: "dichromat" / "honeybee" / "honeybee_mst" / "plane" name the ops that stream through
    run_video as they are; "frame" is every other species.  Of those Cat streams too, through an operator of its own
    (WideStreamOp: has_stream_op, stream_op), as does every dichromat built with fov= (its route() keeps the value it has without);
    the rest run visualize() per frame."""
    from .animals import Cat, HoneyBee
    from .animals._dichromats import _Dichromat
    from .animals._uv_species import UVSpecies
    from .animals.rat_uv import RatUV

    if isinstance(animal, _Dichromat) and not isinstance(animal, Cat):
        return "dichromat"
    if isinstance(animal, HoneyBee) and animal.hsi_model is not None:
        return "honeybee_mst"
    if isinstance(animal, HoneyBee) and not animal.hsi_downsample:
        return "honeybee"
    if isinstance(animal, UVSpecies) and not isinstance(animal, RatUV):
        return "plane"
    return "frame"


def has_stream_op(animal) -> bool:
    """Whether stream_op gives `animal` an operator for run_video (and so --batch, --depth and payload I/O): every route but
    "frame", Cat, and any dichromat with a field of view (fov=)."""
    from .animals import Cat

    return isinstance(animal, Cat) or getattr(animal, "fov", None) is not None or route(animal) != "frame"


def stream_op(animal, H: int, W: int, depth: int, batch: int = 1):
    """The op run_video streams for `animal`, or None when the species goes through the per-frame loop.  batch: frames per
    pipeline slot -- the plane-program species record their plans for that many frames; the dichromat and honeybee ops take
    n_frames per call as they are; the wide view's operator (Cat, or fov=) holds `batch` frames per slot; a species of the
    per-frame loop cannot batch (ValueError)."""
    from .animals import Cat

    if isinstance(animal, Cat) or getattr(animal, "fov", None) is not None:
        from .animals._dichromats import CatStreamOp, WideStreamOp

        return (CatStreamOp if isinstance(animal, Cat) else WideStreamOp)(animal, H, W, depth=depth, batch=batch)
    kind = route(animal)
    if kind in ("dichromat", "honeybee"):
        return animal._operator()
    if kind == "honeybee_mst":  # the network per frame on the slot's stream; ValueError when hsi_scale leaves too small a frame
        from .ml import MstHoneybeeStreamOp

        down = animal.hsi_downsample and 0.05 <= animal.hsi_scale < 1.0
        return MstHoneybeeStreamOp(animal.hsi_model, animal._operator(), H, W, depth=depth, hsi_scale=animal.hsi_scale if down else None, batch=batch)
    if kind == "plane":
        from .animals._uv_species import SpeciesStreamOp

        return SpeciesStreamOp(animal, H, W, depth=depth, batch=batch)
    if batch > 1:
        raise ValueError(f"{type(animal).__name__} runs visualize() per frame: it has no batched form (--batch {batch})")
    return None


def _batch_arg(text: str) -> int:
    from ._lib import AVX_EW_MAX_FRAMES

    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--batch takes an integer (got {text!r})")
    if not 1 <= v <= AVX_EW_MAX_FRAMES:
        raise argparse.ArgumentTypeError(f"--batch must be 1..{AVX_EW_MAX_FRAMES} (got {v})")
    return v


def _hsi_scale_arg(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--hsi-scale takes a number (got {text!r})")
    if not 0.05 <= v < 1.0:  # HoneyBee's own range (honeybee.py:109): outside it the flag would be ignored
        raise argparse.ArgumentTypeError(f"--hsi-scale must be at least 0.05 and below 1 (got {text!r})")
    return v


def _bloom_arg(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--bloom takes a number (got {text!r})")
    if not 0.0 < v <= 1.0:  # (also refuses nan)
        raise argparse.ArgumentTypeError(f"--bloom must be above 0 and at most 1 (got {text!r})")
    return v


def _night_threshold_arg(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--night-threshold takes a number (got {text!r})")
    if not 0.0 <= v <= 1.0:  # (also refuses nan)
        raise argparse.ArgumentTypeError(f"--night-threshold must be at least 0 and at most 1 (got {text!r})")
    return v


def _fov_arg(text: str):
    try:
        phi, overlap = (float(v) for v in text.split(":"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--fov takes PHI:OVERLAP in degrees, e.g. 105:40 (got {text!r})")
    if not 0.0 < phi <= 180.0:  # (also refuses nan)
        raise argparse.ArgumentTypeError(f"--fov: PHI must be above 0 and at most 180 (got {text!r})")
    if not 0.0 <= overlap <= 360.0:
        raise argparse.ArgumentTypeError(f"--fov: OVERLAP must be at least 0 and at most 360 (got {text!r})")
    return phi, overlap


def _camera_hfov_arg(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--camera-hfov takes a number (got {text!r})")
    if not 0.0 < v < 180.0:  # (also refuses nan)
        raise argparse.ArgumentTypeError(f"--camera-hfov must be above 0 and below 180 (got {text!r})")
    return v


def _fov_ratio_arg(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--fov-ratio takes a number (got {text!r})")
    if not (math.isfinite(v) and v >= 1.0):
        raise argparse.ArgumentTypeError(f"--fov-ratio must be finite and at least 1 (got {text!r})")
    return v


def is_dichromat(species: str) -> bool:
    """Whether the display name is one of the 20 dichromats, the species that have a night form."""
    from .animals._dichromats import _Dichromat

    return issubclass(species_class(species), _Dichromat)


def _wxh_arg(flag: str, example: str):
    def parse(text: str):
        try:
            w, h = (int(v) for v in text.lower().split("x"))
        except ValueError:
            raise argparse.ArgumentTypeError(f"{flag} takes WxH, e.g. {example} (got {text!r})")
        if w < 1 or h < 1:
            raise argparse.ArgumentTypeError(f"{flag} must be positive (got {text!r})")
        return w, h

    return parse


_size_arg = _wxh_arg("--size", "3840x2160")
_scale_arg = _wxh_arg("--scale", "1920x1080")


def check_io_options(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """The checks of the I/O options that depend on each other (the HDR ones, `--matrix bt2020`, `--scale` against a size the
    command line names), with their defaults filled in; shared by the `video` and `wall` commands.  Errors go through ap.error."""
    if args.transfer is not None:
        from .yuv import HDR_PIX_FMTS

        if args.pix_fmt not in HDR_PIX_FMTS:
            ap.error(f"--transfer needs --pix-fmt naming a 10-bit format ({', '.join(HDR_PIX_FMTS)}); got --pix-fmt {args.pix_fmt}")
        if args.matrix not in (None, "bt2020"):
            ap.error(f"--matrix {args.matrix} with --transfer: HDR video is decoded with the bt2020 matrix (--out-matrix names the output's)")
    else:
        if args.matrix == "bt2020":
            ap.error("--matrix bt2020 needs --transfer: bt2020 is decoded on the HDR path only")
        for flag, v in (("--tonemap", args.tonemap), ("--peak-nits", args.peak_nits), ("--sdr-white", args.sdr_white)):
            if v is not None:
                ap.error(f"{flag} needs --transfer")
    args.tonemap = args.tonemap or "mobius"
    args.peak_nits = 1000.0 if args.peak_nits is None else args.peak_nits
    args.sdr_white = 203.0 if args.sdr_white is None else args.sdr_white
    if not (math.isfinite(args.peak_nits) and math.isfinite(args.sdr_white) and args.sdr_white > 0.0 and args.peak_nits > args.sdr_white):
        ap.error(f"--peak-nits and --sdr-white must be finite and positive, with --peak-nits above --sdr-white (got {args.peak_nits} and {args.sdr_white})")
    if args.matrix is None or args.transfer is not None:
        args.matrix = "bt601"  # what the SDR conversions use; the HDR decode takes no matrix
    src = args.size  # the source's size where the command line names it: --size, or a synthetic: input
    if src is None and args.input.startswith("synthetic:"):
        try:
            src = _size_arg(args.input.split(":")[1])
        except (IndexError, argparse.ArgumentTypeError):
            src = None
    if args.scale is not None and src is not None and (args.scale[0] > src[0] or args.scale[1] > src[1]):
        ap.error(f"--scale {args.scale[0]}x{args.scale[1]} enlarges the {src[0]}x{src[1]} source: --scale only reduces")


def check_raw_options(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """`--pix-fmt` and `--size` name raw video only together."""
    if (args.pix_fmt is None) != (args.size is None):
        ap.error("--pix-fmt and --size go together: raw video carries neither its format nor its size")


class _VideoParser(argparse.ArgumentParser):
    """The command's parser; parse_args also checks the options that depend on each other (the HDR ones, `--matrix bt2020`)."""

    def parse_args(self, args=None, namespace=None):
        args = super().parse_args(args, namespace)
        for flag, v in (("--hsi-model", args.hsi_model), ("--hsi-scale", args.hsi_scale)):
            if v is not None and args.species != "HoneyBee":
                self.error(f"{flag} configures HoneyBee's RGB-to-spectrum conversion: --species {args.species} has none")
        night, bloom = getattr(args, "night", False), getattr(args, "bloom", None)  # (add_night_options: parse_args adds them)
        auto, threshold = getattr(args, "night_auto", False), getattr(args, "night_threshold", None)
        if night and auto:
            self.error("--night and --night-auto exclude each other: --night is night for every frame, --night-auto decides per frame")
        if threshold is not None and not auto:
            self.error("--night-threshold needs --night-auto: it is the median luma below which --night-auto calls a frame night")
        if bloom is not None and not (night or auto):
            self.error("--bloom needs --night: the tapetum bloom is part of the night view")
        if night and not is_dichromat(args.species):
            self.error(f"--night: --species {args.species} is not one of the 20 dichromats, the species that have a night view")
        if auto and not is_dichromat(args.species):
            self.error(f"--night-auto: --species {args.species} is not one of the 20 dichromats, the species that have a night view")
        fov = getattr(args, "fov", None)  # (add_fov_options: parse_args adds them)
        for flag, v in (("--camera-hfov", getattr(args, "camera_hfov", None)), ("--fov-ratio", getattr(args, "fov_ratio", None))):
            if v is not None and fov is None:
                self.error(f"{flag} needs --fov: it is part of the wide view's geometry")
        if fov is not None and not is_dichromat(args.species):
            self.error(f"--fov: --species {args.species} is not one of the 20 dichromats, the species that have a wide view")
        if args.hsi_model not in (None, "seeded") and not os.path.isfile(args.hsi_model):
            self.error(f"--hsi-model {args.hsi_model}: no such file (a local .pth checkpoint, or 'seeded')")
        check_io_options(self, args)
        return args


def add_io_arguments(ap: argparse.ArgumentParser) -> None:
    """INPUT and OUTPUT, as the `video` and `wall` commands take them."""
    ap.add_argument("input", help=".y4m file, '-' (stdin: Y4M, or raw video with --pix-fmt), a raw video file (--pix-fmt), "
                                  "synthetic:<W>x<H>:<n>[:kind], .npy or an image directory")
    ap.add_argument("output", help=".y4m file, '-' (stdout: Y4M, or raw video with --pix-fmt / --out-pix-fmt), a raw video file, .npy or a "
                                   "directory of PNG frames")


def add_input_options(ap: argparse.ArgumentParser) -> None:
    """The options of the frame pipeline and of the input side (--depth ... --scale), shared by `video` and `wall`."""
    ap.add_argument("--depth", type=int, default=3, help="frames in flight on the device (streamed species)")
    ap.add_argument("--batch", type=_batch_arg, default=1, metavar="N", help="frames per slot and per launch chain, 1..16 (streamed species only)")
    ap.add_argument("--matrix", default=None, choices=["bt601", "bt709", "bt2020"],
                    help="YUV matrix (default bt601); with --transfer the decode is always bt2020, and only that may be named")
    ap.add_argument("--range", default=None, choices=["limited", "full"], help="YUV range (default: the input's XCOLORRANGE, else limited)")
    ap.add_argument("--pix-fmt", default=None, choices=list(AVX_PIX_FMTS), metavar="NAME",
                    help="read INPUT as raw video in this format (ffmpeg's -pix_fmt names: " + ", ".join(AVX_PIX_FMTS) + "); needs --size")
    ap.add_argument("--size", default=None, type=_size_arg, metavar="WxH", help="frame size of the raw input")
    ap.add_argument("--scale", default=None, type=_scale_arg, metavar="WxH",
                    help="reduce every frame to this size on the device as it is decoded (INTER_AREA; never enlarges); the species and OUTPUT "
                         "have this size")


def add_output_options(ap: argparse.ArgumentParser) -> None:
    """The options of the HDR decode and of the output side (--out-pix-fmt ... --out-matrix), shared by `video` and `wall`."""
    ap.add_argument("--out-pix-fmt", default=None, choices=list(AVX_PIX_FMTS), metavar="NAME",
                    help="write OUTPUT as raw video in this format (default: --pix-fmt when OUTPUT is '-' or ends in .yuv)")
    ap.add_argument("--transfer", default=None, choices=list(AVX_TRANSFERS),
                    help="read INPUT as HDR video (BT.2020) with this transfer function and tone-map it to SDR; needs a 10-bit --pix-fmt")
    ap.add_argument("--tonemap", default=None, choices=list(AVX_TONEMAPS), help="tone curve of --transfer (default mobius)")
    ap.add_argument("--peak-nits", default=None, type=float, metavar="X", help="the clip's peak luminance, mapped to SDR white (default 1000)")
    ap.add_argument("--sdr-white", default=None, type=float, metavar="X", help="the luminance shown as SDR white (default 203, BT.2408)")
    ap.add_argument("--out-matrix", default=None, choices=["bt601", "bt709"],
                    help="YUV matrix of the output (default: bt709 with --transfer, else --matrix)")


def build_parser() -> argparse.ArgumentParser:
    ap = _VideoParser(prog="video", description="Run one species on every frame of a video (Y4M in and out, or the other VideoRenderer forms).")
    add_io_arguments(ap)
    ap.add_argument("--species", required=True, choices=SPECIES_NAMES, metavar="NAME", help="display name, e.g. Dog, HoneyBee, 'Mantis Shrimp'")
    ap.add_argument("--split-compare", action="store_true", help="left half original, right half transformed (the reference's output)")
    ap.add_argument("--no-labels", action="store_true", help="no corner labels on the split frame")
    add_input_options(ap)
    ap.add_argument("--hsi-model", default=None, metavar="seeded|PATH",
                    help="HoneyBee only: take the 31-band cube from the MST++ network instead of the analytic lobes.  PATH is a local .pth "
                         "checkpoint of the reference's MST++ (its state_dict / module. form); no checkpoint ships with this package, and "
                         "'seeded' (random weights from a fixed seed) is for testing")
    ap.add_argument("--hsi-scale", default=None, type=_hsi_scale_arg, metavar="S",
                    help="HoneyBee only, 0.05 <= S < 1: convert RGB to spectrum on the frame reduced by S and enlarge the three cone catches "
                         "(hsi_downsample).  With --hsi-model the network runs at the reduced size: a stated quality-for-speed choice")
    add_output_options(ap)
    return ap


def add_night_options(ap: argparse.ArgumentParser) -> None:
    """--night and --bloom.  parse_args adds them to build_parser()'s parser: build_parser() itself stays the option
    list and help text that tests/golden/video_parser.json records."""
    ap.add_argument("--night", action="store_true",
                    help="the dichromats only: rod vision (scotopic luminance, desaturation, boost, gamma) in front of the species' colour stage")
    ap.add_argument("--bloom", default=None, type=_bloom_arg, metavar="S",
                    help="with --night, 0 < S <= 1: tapetum bloom of this strength (a luminance-gated screen blend with a sigma 3 blur)")


def add_night_auto_options(ap: argparse.ArgumentParser) -> None:
    """--night-auto and --night-threshold, added by parse_args like add_night_options."""
    ap.add_argument("--night-auto", action="store_true",
                    help="the dichromats only: decide per frame -- the night view (with --bloom S its bloom) where the frame's median Rec.709 luma "
                         "is below the threshold, the day view elsewhere")
    ap.add_argument("--night-threshold", default=None, type=_night_threshold_arg, metavar="T",
                    help="with --night-auto, 0 <= T <= 1: the median luma below which a frame is night (default 0.12)")


def add_fov_options(ap: argparse.ArgumentParser) -> None:
    """--fov, --camera-hfov and --fov-ratio, added by parse_args like add_night_options."""
    ap.add_argument("--fov", default=None, type=_fov_arg, metavar="PHI:OVERLAP",
                    help="the dichromats only: the binocular wide view, e.g. 105:40 -- each eye sees PHI degrees to either side of its axis, "
                         "the two fields share OVERLAP degrees; the output spans 4 PHI - OVERLAP degrees and --split-compare's left half is "
                         "the centre-zoomed input")
    ap.add_argument("--camera-hfov", default=None, type=_camera_hfov_arg, metavar="DEG",
                    help="with --fov, 0 < DEG < 180: the horizontal field the camera's frame covers (default 100)")
    ap.add_argument("--fov-ratio", default=None, type=_fov_ratio_arg, metavar="R",
                    help="with --fov, R >= 1: how much wider the animal's field is than the human's the baseline is zoomed to (default 1.30)")


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = build_parser()
    add_night_options(ap)
    add_night_auto_options(ap)
    add_fov_options(ap)
    args = ap.parse_args(argv)
    check_raw_options(ap, args)
    return args


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    if args.depth < 1:
        raise SystemExit("video: --depth must be at least 1")
    from .pipeline import run_video
    from .renderers import VideoRenderer, split_compose

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
        raise SystemExit(f"video: --scale {args.scale[0]}x{args.scale[1]}: {e}")  # a .y4m header smaller than --scale
    animal = make_animal(args)
    if args.batch > 1 and not has_stream_op(animal):  # before any frame is read
        vr.close()
        raise SystemExit(f"video: --batch {args.batch}: {args.species} runs visualize() per frame and has no batched form")
    labels = None if args.no_labels else ("Original", "Transformed")
    auto_counts = [0, 0]  # --night-auto: night frames, frames (the stream op counts them)
    t0 = time.perf_counter()
    try:
        hw = None if vr.y4m_header is None else (vr.y4m_header.height, vr.y4m_header.width)
        if args.size is not None:
            hw = (args.size[1], args.size[0])
        if hw is not None and args.scale is not None:
            hw = (args.scale[1], args.scale[0])  # what the species runs on
        if hw is None:  # synthetic:, .npy or an image directory: peek at the size the stream op is built for, then start over
            first = vr.get_image()
            hw = None if first is None else first.shape[:2]
            vr.close()
            vr = renderer()
            vr.open()
        try:
            op = None if hw is None else stream_op(animal, hw[0], hw[1], args.depth, args.batch)
        except ValueError as e:
            if args.hsi_scale is None or "hsi_scale" not in str(e):
                raise
            raise SystemExit(f"video: --hsi-scale {args.hsi_scale:g}: {e}")  # the reduced frame is too small for the network
        if op is not None:
            try:
                # the split frame's left half is visualize()'s baseline: the input for the dichromats and HoneyBee, the
                # panorama-warped input for the plane-program species (their plans' baseline frames), the zoomed input for Cat
                stats = run_video(op, vr, depth=args.depth, split_compare=args.split_compare, labels=labels,
                                  split_baseline=hasattr(op, "slot_baseline"), batch=args.batch)
            finally:
                auto_counts = list(getattr(op, "auto_counts", auto_counts))
                if hasattr(op, "close"):
                    op.close()
            frames = stats.frames
        else:
            frames = 0
            while True:
                frame = vr.get_image()
                if frame is None:
                    break
                res = animal.visualize(frame)
                if res is None:
                    continue
                base, out = res
                if out is None:
                    continue
                base, out = ensure_rgb_uint8(np.asarray(base)), ensure_rgb_uint8(np.asarray(out))
                if args.split_compare:
                    vr.render(split_compose(base, out, left_label=labels[0] if labels else None, right_label=labels[1] if labels else None))
                else:
                    vr.render(out)
                frames += 1
    finally:
        vr.close()
    dt = time.perf_counter() - t0
    print(f"video: {args.species}: {frames} frames in {dt:.2f} s ({frames / dt if dt > 0 else 0.0:.1f} fps)", file=sys.stderr)
    if getattr(args, "night_auto", False):
        k, n = auto_counts
        print(f"night-auto: {k} of {n} frames night (threshold {animal.night.threshold:g})", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
