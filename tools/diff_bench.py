"""Time of the difference-map kernels.  Not part of bench.py.

  python tools/diff_bench.py kernel [--reps 7]
      avx_diff_map_u8 on frames resident on the device, 1080p and 4K, batches of 8: the abs, heat and ssim modes, each in the map and
      the side layout, interleaved in one process with avx_frame_metrics_u8(with_ssim = 1) on the same frames -- per repetition each
      of the seven forms once, each between its own pair of stream events (the record memset and the final launch included), after one
      warm-up call of each.  One JSON line per (size, mode, layout): median (min-max) in us per frame.  For abs and heat also what the
      bytes the kernel moves (both inputs and the output: 9 B/px for map, 15 B/px for side) would take at 6.29 TB/s (the measured HBM
      copy rate, MI355X) and the share of that rate reached; for ssim the ratio to the SSIM record kernel, which runs the same passes
      plus the histogram and stores no pixels.  The frames are noise against the same noise +-2 codes: most differences are 0, 1 or 2,
      as between two renderings of one clip.
  python tools/diff_bench.py command [--frames 32] [--reps 3] [--dir DIR]
      Two 4K nv12 files of `frames` frames in DIR (default: /dev/shm when there is one, so they are read from and written to memory)
      through python -m animal_vision_amd.diff's main(), --batch 8 --depth 2: heat into a raw nv12 file (the map encoded on the device,
      1.5 B/px back across PCIe), heat side by side into nv12, ssim into nv12, and heat into a .npy file (RGB, 3 B/px back): frames per
      second of the whole command (read, upload, decode, map, encode, download, write), `reps` runs each after one warm-up run."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

COPY_BPS = 6.29e12
SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}


def _pair(n, H, W, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-2, 3, a.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    return a, b


def kernel(args):
    from animal_vision_amd.metrics import DIFF_RECORD_BYTES, RECORD_BYTES, diff_map_launch, frame_metrics_launch
    from animal_vision_amd.runtime import get_context

    ctx, n = get_context(), 8
    for name, (H, W) in (("4k", SIZES["4k"]), ("1080p", SIZES["1080p"])):
        a, b = _pair(n, H, W)
        d_a, d_b, d_out = ctx.upload(a), ctx.upload(b), ctx.malloc(3 * n * H * W * 3)
        d_rec, d_metrics = ctx.malloc(n * DIFF_RECORD_BYTES), ctx.malloc(n * RECORD_BYTES)

        def diff_route(mode, layout):
            return lambda: diff_map_launch(ctx, d_a, d_b, n, H, W, d_out, d_rec, mode=mode, threshold=1, layout=layout)

        forms = [(mode, layout, diff_route(mode, layout)) for mode in ("abs", "heat", "ssim") for layout in ("map", "side")]
        forms.append(("record", None, lambda: frame_metrics_launch(ctx, d_a, d_b, n, H, W, d_metrics, ssim=True)))
        times = [[] for _ in forms]
        for _, _, route in forms:  # warm-up: code objects are loaded and the record kernel's workspace is sized here
            route()
        ctx.sync()
        for _ in range(args.reps):
            for k, (_, _, route) in enumerate(forms):
                ctx.timer_start()
                route()
                times[k].append(ctx.timer_stop() * 1e3 / n)
        record = float(np.median(times[-1]))
        for (mode, layout, _), t in zip(forms, times):
            line = {"size": name, "mode": mode, "layout": layout, "batch": n, "reps": args.reps, "us_per_frame_median": round(float(np.median(t)), 1),
                    "us_per_frame_min": round(min(t), 1), "us_per_frame_max": round(max(t), 1)}
            if mode in ("abs", "heat"):
                floor = (15.0 if layout == "side" else 9.0) * H * W / COPY_BPS * 1e6
                line.update({"bytes_per_px": 15 if layout == "side" else 9, "us_those_bytes_at_6.29TBps": round(floor, 1),
                             "share_of_copy_rate": round(floor / float(np.median(t)), 3)})
            elif mode == "ssim":
                line["over_ssim_record_kernel"] = round(float(np.median(t)) / record, 2)
            print(json.dumps(line), flush=True)
        for d in (d_a, d_b, d_out, d_rec, d_metrics):
            d.free()


def command(args):
    from animal_vision_amd import diff
    from animal_vision_amd.yuv import rgb_to_yuv

    H, W = SIZES["4k"]
    base = args.dir or ("/dev/shm" if os.path.isdir("/dev/shm") else None)
    with tempfile.TemporaryDirectory(dir=base) as d:
        a, b = _pair(4, H, W)
        pa, pb = [rgb_to_yuv(f, pix_fmt="nv12") for f in a], [rgb_to_yuv(f, pix_fmt="nv12") for f in b]
        for path, pay in ((os.path.join(d, "a.yuv"), pa), (os.path.join(d, "b.yuv"), pb)):
            with open(path, "wb") as f:
                for i in range(args.frames):
                    f.write(pay[i % len(pay)].tobytes())
        argv = [os.path.join(d, "a.yuv"), os.path.join(d, "b.yuv")]
        opts = ["--pix-fmt", "nv12", "--size", f"{W}x{H}", "--batch", "8", "--depth", "2"]
        for out, extra in (("out.yuv", []), ("out.yuv", ["--layout", "side"]), ("out.yuv", ["--mode", "ssim"]), ("out.npy", [])):
            fps = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                with contextlib.redirect_stderr(io.StringIO()):
                    status = diff.main(argv + [os.path.join(d, out)] + opts + extra)
                dt = time.perf_counter() - t0
                assert status == 0, status
                os.remove(os.path.join(d, out))
                if rep:  # the first run is the warm-up
                    fps.append(args.frames / dt)
            print(json.dumps({"command": "diff", "size": "4k", "pix_fmt": "nv12", "frames": args.frames, "batch": 8, "depth": 2,
                              "sink": "nv12" if out.endswith(".yuv") else "npy", "options": extra, "reps": args.reps,
                              "fps_median": round(float(np.median(fps)), 1), "fps_min": round(min(fps), 1), "fps_max": round(max(fps), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--reps", type=int, default=7)
    c = sub.add_parser("command")
    c.add_argument("--frames", type=int, default=32)
    c.add_argument("--reps", type=int, default=3)
    c.add_argument("--dir", default=None)
    args = ap.parse_args()
    {"kernel": kernel, "command": command}[args.cmd](args)


if __name__ == "__main__":
    main()
