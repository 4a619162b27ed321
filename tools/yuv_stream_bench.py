"""I420 vs RGB host I/O of the 4K dog stream, and the YUV kernels' time per 4K frame.  Not part of bench.py.

  python tools/yuv_stream_bench.py stream  [--frames 256] [--distinct 32] [--reps 3]
      The dog stream at 3840x2160 with split-compare through FramePipeline (depth 3), fed from frames held in memory (`distinct`
      frames cycled, converted beforehand, so no disk or decode bounds it): io_format="rgb" and "i420" alternately, `reps`
      times each after one warm-up run each.  One JSON line per run: frames/s and host_copy_s.
  python tools/yuv_stream_bench.py kernels [--iters 20]
      8-frame 4K batches through avx_i420_to_rgb_u8 and avx_rgb_to_i420_u8, for `rocprofv3 --kernel-trace --stats` to time.
  python tools/yuv_stream_bench.py report STATS_CSV
      The kernels' mean time per 4K frame from rocprofv3's kernel_stats.csv, and its share of 6.29 TB/s (the measured HBM copy
      rate, MI355X) for the 4.5 B/px each direction moves."""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

H, W = 2160, 3840
COPY_BPS = 6.29e12


def stream(args):
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.synthetic import structured_frame
    from animal_vision_amd.yuv import rgb_to_i420

    rgb = [structured_frame(k, H, W) for k in range(args.distinct)]
    yuv = [rgb_to_i420(f) for f in rgb]
    src = {"rgb": rgb, "i420": yuv}

    def run(fmt, n):
        pipe = FramePipeline(DichromatOp(Dog.SPEC), H, W, depth=3, split_compare=True, io_format=fmt)
        try:
            frames = src[fmt]
            st = pipe.run(((i, frames[i % len(frames)]) for i in range(n)), lambda i, o: None)
        finally:
            pipe.close()
        return st

    for fmt in ("rgb", "i420"):
        run(fmt, 16)
    for rep in range(args.reps):
        for fmt in ("rgb", "i420"):
            st = run(fmt, args.frames)
            print(json.dumps({"io_format": fmt, "rep": rep, "frames": st.frames, "seconds": round(st.seconds, 4),
                              "fps": round(st.frames / st.seconds, 1), "host_copy_s": round(st.host_copy_seconds, 4)}), flush=True)


def kernels(args):
    from animal_vision_amd.runtime import get_context
    from animal_vision_amd.yuv import i420_size, i420_to_rgb_device, rgb_to_i420_device

    ctx = get_context()
    n = 8
    d_rgb, d_yuv, d_rgb2 = ctx.malloc(n * H * W * 3), ctx.malloc(n * i420_size(H, W)), ctx.malloc(n * H * W * 3)
    rng = np.random.default_rng(0)
    ctx.upload(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), d_rgb)
    for _ in range(args.iters):
        rgb_to_i420_device(ctx, d_rgb, d_yuv, n, H, W)
        i420_to_rgb_device(ctx, d_yuv, d_rgb2, n, H, W)
    ctx.sync()
    print(json.dumps({"kernels": "done", "iters": args.iters, "batch": n}))
    for d in (d_rgb, d_yuv, d_rgb2):
        d.free()


def report(args):
    bytes_per_frame = 4.5 * H * W  # 1.5 B/px of I420 + 3 B/px of RGB, in one direction
    with open(args.csv) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "i420" not in name:
                continue
            avg_ns = float(row.get("AverageNs") or row.get("Average") or 0.0)
            us = avg_ns / 1e3 / 8
            kernel = re.search(r"k_\w+", name)
            print(json.dumps({"kernel": kernel.group(0) if kernel else name, "calls": int(row.get("Calls", 0)), "us_per_4k_frame": round(us, 2),
                              "TB_per_s": round(bytes_per_frame / (us * 1e-6) / 1e12, 3),
                              "frac_of_6.29TBps": round(bytes_per_frame / COPY_BPS / (us * 1e-6), 3)}))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("stream")
    s.add_argument("--frames", type=int, default=256)
    s.add_argument("--distinct", type=int, default=32)
    s.add_argument("--reps", type=int, default=3)
    k = sub.add_parser("kernels")
    k.add_argument("--iters", type=int, default=20)
    r = sub.add_parser("report")
    r.add_argument("csv")
    args = ap.parse_args()
    {"stream": stream, "kernels": kernels, "report": report}[args.cmd](args)


if __name__ == "__main__":
    main()
