"""I420 vs RGB host I/O of the 4K dog stream, and the YUV kernels' time per 4K frame.  Not part of bench.py.

  python tools/yuv_stream_bench.py stream  [--frames 256] [--distinct 32] [--reps 3] [--pix-fmt NAME ...]
      The dog stream at 3840x2160 with split-compare through FramePipeline (depth 3), fed from frames held in memory (`distinct`
      frames cycled, converted beforehand, so no disk or decode bounds it): io_format="rgb" and "i420" alternately, `reps`
      times each after one warm-up run each.  One JSON line per run: frames/s and host_copy_s.  With --pix-fmt the runs are
      io_format="i420" (the baseline) and io_format="yuv" in every named raw format instead.
  python tools/yuv_stream_bench.py kernels [--iters 20] [--pix-fmt NAME ...] [--transfer NAME ...] [--scale WxH]
      8-frame 4K batches through avx_i420_to_rgb_u8 and avx_rgb_to_i420_u8, for `rocprofv3 --kernel-trace --stats` to time; with
      --pix-fmt, also through avx_yuv_to_rgb_u8 and avx_rgb_to_yuv_u8 in every named format, in the same process; with
      --transfer pq hlg, every named 10-bit format also goes through avx_yuv_hdr_to_rgb_u8 with each transfer (the HDR decode of
      §4.10), beside the SDR decode of the same payload; with --scale WxH, every named format also goes through the scaled decode
      of §4.11 (avx_yuv_to_rgb_scaled_u8, one launch per batch) and, in the same process, through the chain it replaces:
      avx_yuv_to_rgb_u8 on the batch, then one avx_resize_hwc (uint8, INTER_AREA) per frame.  One JSON line per format carries
      both as timed with stream events around the `iters` repetitions (launch gaps included).  With both --transfer and --scale,
      every named 10-bit format and transfer also goes through the scaled HDR decode of §4.13 (avx_yuv_hdr_to_rgb_scaled_u8, one
      launch per batch) and through the chain it replaces -- avx_yuv_hdr_to_rgb_u8 on the batch, then one avx_resize_hwc per
      frame -- on the same payloads; each of the `iters` repetitions is timed with its own pair of stream events, and the JSON
      line carries the medians and chain_over_fused.
  python tools/yuv_stream_bench.py report STATS_CSV [--transfer NAME ...] [--scale WxH]
      The kernels' mean time per 4K frame from rocprofv3's kernel_stats.csv, and its share of 6.29 TB/s (the measured HBM copy
      rate, MI355X) for the bytes each direction moves: the format's B/px plus 3 B/px of RGB.  An HDR decode kernel's line also
      carries its transfer and its time over the SDR decode kernel's of the same format in the same run (both move the same
      bytes, so the ratio is arithmetic); --transfer keeps only the named transfers' HDR lines.  A scaled decode kernel's line
      carries its time per 4K source frame, the chain's in the same run (the plain decode kernel of the format plus the uint8
      INTER_AREA resize kernel, kernel time only) and chain / fused; a scaled HDR decode kernel's line (§4.13) the same beside
      the HDR decode kernel of its format and transfer plus the resize kernel, and with --scale WxH (the run's) its share of
      6.29 TB/s for the payload in plus 3 B per destination pixel out."""
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

    from animal_vision_amd.yuv import rgb_to_yuv

    rgb = [structured_frame(k, H, W) for k in range(args.distinct)]
    src = {"i420": [rgb_to_i420(f) for f in rgb]}
    if args.pix_fmt:
        for p in args.pix_fmt:
            src[p] = [rgb_to_yuv(f, pix_fmt=p) for f in rgb]
    else:
        src = {"rgb": rgb, **src}

    def run(fmt, n):
        raw = fmt not in ("rgb", "i420")
        pipe = FramePipeline(DichromatOp(Dog.SPEC), H, W, depth=3, split_compare=True, io_format="yuv" if raw else fmt, pix_fmt=fmt if raw else None)
        try:
            frames = src[fmt]
            st = pipe.run(((i, frames[i % len(frames)]) for i in range(n)), lambda i, o: None)
        finally:
            pipe.close()
        return st

    for fmt in src:
        run(fmt, 16)
    for rep in range(args.reps):
        for fmt in src:
            st = run(fmt, args.frames)
            print(json.dumps({"io_format": fmt, "rep": rep, "frames": st.frames, "seconds": round(st.seconds, 4),
                              "fps": round(st.frames / st.seconds, 1), "host_copy_s": round(st.host_copy_seconds, 4)}), flush=True)


def kernels(args):
    from animal_vision_amd.runtime import get_context
    from animal_vision_amd.yuv import (HDR_PIX_FMTS, frame_size, i420_size, i420_to_rgb_device, rgb_to_i420_device, rgb_to_yuv_device,
                                       yuv_hdr_to_rgb_device, yuv_hdr_to_rgb_scaled_device, yuv_to_rgb_device, yuv_to_rgb_scaled_device)
    from animal_vision_amd.geometry import INTER_AREA, resize_device

    ctx = get_context()
    n = 8
    d_rgb, d_yuv, d_rgb2 = ctx.malloc(n * H * W * 3), ctx.malloc(n * i420_size(H, W)), ctx.malloc(n * H * W * 3)
    rng = np.random.default_rng(0)
    ctx.upload(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), d_rgb)
    for _ in range(args.iters):
        rgb_to_i420_device(ctx, d_rgb, d_yuv, n, H, W)
        i420_to_rgb_device(ctx, d_yuv, d_rgb2, n, H, W)
    for p in args.pix_fmt or []:
        d_raw = ctx.malloc(n * frame_size(p, H, W))
        for _ in range(args.iters):
            rgb_to_yuv_device(ctx, p, d_rgb, d_raw, n, H, W)
            yuv_to_rgb_device(ctx, p, d_raw, d_rgb2, n, H, W)
        for tr in (args.transfer or []) if p in HDR_PIX_FMTS else []:  # the same payload, read as HDR: the same bytes in and out
            for _ in range(args.iters):
                yuv_hdr_to_rgb_device(ctx, p, d_raw, d_rgb2, n, H, W, transfer=tr)
        if args.scale:
            Wd, Hd = args.scale
            d_small = ctx.malloc(n * Hd * Wd * 3)
            small = [d_small.view(f * Hd * Wd * 3, Hd * Wd * 3) for f in range(n)]
            full = [d_rgb2.view(f * H * W * 3, H * W * 3) for f in range(n)]

            def fused():
                yuv_to_rgb_scaled_device(ctx, p, d_raw, d_small, n, H, W, Hd, Wd)

            def chain():
                yuv_to_rgb_device(ctx, p, d_raw, d_rgb2, n, H, W)
                for f in range(n):
                    resize_device(ctx, full[f], np.uint8, H, W, 3, Hd, Wd, INTER_AREA, small[f])

            ms = {}
            for name, fn in (("fused", fused), ("chain", chain)):
                fn()  # the first call of a geometry builds and uploads its tables
                ctx.sync()
                ctx.timer_start()
                for _ in range(args.iters):
                    fn()
                ms[name] = ctx.timer_stop()
            us = {k: v * 1e3 / (args.iters * n) for k, v in ms.items()}
            print(json.dumps({"scaled_decode": p, "scale": f"{Wd}x{Hd}", "batch": n, "iters": args.iters, "fused_us_per_4k_frame": round(us["fused"], 2),
                              "chain_us_per_4k_frame": round(us["chain"], 2), "chain_over_fused": round(us["chain"] / us["fused"], 2)}), flush=True)
            for tr in (args.transfer or []) if p in HDR_PIX_FMTS else []:  # §4.13: the same payload, read as HDR

                def hdr_fused():
                    yuv_hdr_to_rgb_scaled_device(ctx, p, d_raw, d_small, n, H, W, Hd, Wd, transfer=tr)

                def hdr_chain():
                    yuv_hdr_to_rgb_device(ctx, p, d_raw, d_rgb2, n, H, W, transfer=tr)
                    for f in range(n):
                        resize_device(ctx, full[f], np.uint8, H, W, 3, Hd, Wd, INTER_AREA, small[f])

                med = {}
                for name, fn in (("fused", hdr_fused), ("chain", hdr_chain)):
                    fn()
                    ctx.sync()
                    each = []
                    for _ in range(args.iters):  # every repetition between its own pair of events: the median is quoted
                        ctx.timer_start()
                        fn()
                        each.append(ctx.timer_stop())
                    med[name] = float(np.median(each)) * 1e3 / n
                print(json.dumps({"scaled_hdr_decode": p, "transfer": tr, "scale": f"{Wd}x{Hd}", "batch": n, "iters": args.iters,
                                  "fused_us_per_4k_frame": round(med["fused"], 2), "chain_us_per_4k_frame": round(med["chain"], 2),
                                  "chain_over_fused": round(med["chain"] / med["fused"], 2)}), flush=True)
            d_small.free()
        ctx.sync()
        d_raw.free()
    ctx.sync()
    print(json.dumps({"kernels": "done", "iters": args.iters, "batch": n, "pix_fmt": args.pix_fmt or [], "transfer": args.transfer or []}))
    for d in (d_rgb, d_yuv, d_rgb2):
        d.free()


# the template arguments of csrc/yuv_raw.hip's Fmt<T, SX, SY, IL, SH, LUMA>, as they appear in a demangled kernel name
_RAW_FMT = {("unsigned char", 1, 1, False, 0, False): "yuv420p", ("unsigned char", 1, 1, True, 0, False): "nv12",
            ("unsigned char", 1, 0, False, 0, False): "yuv422p", ("unsigned char", 0, 0, False, 0, False): "yuv444p",
            ("unsigned char", 0, 0, False, 0, True): "gray", ("unsigned short", 1, 1, False, 0, False): "yuv420p10le",
            ("unsigned short", 1, 0, False, 0, False): "yuv422p10le", ("unsigned short", 0, 0, False, 0, False): "yuv444p10le",
            ("unsigned short", 1, 1, True, 6, False): "p010le"}


def _raw_fmt_of(name):
    m = re.search(r"Fmt<(unsigned char|unsigned short), (\d+), (\d+), (true|false), (\d+), (true|false)>", name)
    if not m:
        return None
    return _RAW_FMT.get((m.group(1), int(m.group(2)), int(m.group(3)), m.group(4) == "true", int(m.group(5)), m.group(6) == "true"))


_TRANSFER = {1: "pq", 2: "hlg"}  # enum avx_transfer: the HDR kernels' template argument after the format


def report(args):
    from animal_vision_amd.yuv import frame_size

    rows = []
    resize_us = None  # the uint8 INTER_AREA resize kernel: one call per frame, whatever the format
    with open(args.csv) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if re.search(r"k_resize_area(_fast)?_f32<unsigned char>", name):
                resize_us = float(row.get("AverageNs") or row.get("Average") or 0.0) / 1e3
            fmt = "yuv420p" if "i420" in name else _raw_fmt_of(name)
            if fmt is None:
                continue
            kernel = re.search(r"k_\w+", name)
            hdr = re.search(r"_hdr_to_rgb_\w+<.*?Fmt<[^>]*>, (\d+)", name)
            avg_ns = float(row.get("AverageNs") or row.get("Average") or 0.0)
            rows.append({"kernel": kernel.group(0) if kernel else name, "pix_fmt": "i420" if "i420" in name else fmt,
                         "transfer": _TRANSFER.get(int(hdr.group(1))) if hdr else None, "calls": int(row.get("Calls", 0)), "us": avg_ns / 1e3 / 8})
    scaled = ("k_yuv420_to_rgb_half_vec", "k_yuv_to_rgb_area_int", "k_yuv_to_rgb_area_gen")  # csrc/yuv_scale.hip
    scaled_hdr = ("k_yuv420_hdr_to_rgb_half_vec", "k_yuv_hdr_to_rgb_area_int", "k_yuv_hdr_to_rgb_area_gen")  # csrc/yuv_hdr_scale.hip
    hdr_us = {(r["pix_fmt"], r["transfer"]): r["us"] for r in rows if r["transfer"] is not None and r["kernel"] not in scaled_hdr}
    sdr = {r["pix_fmt"]: r["us"] for r in rows
           if r["transfer"] is None and "_to_rgb" in r["kernel"] and r["pix_fmt"] != "i420" and r["kernel"] not in scaled}
    for r in rows:
        if r["kernel"] in scaled:  # beside the chain it replaces: the format's plain decode kernel + the resize kernel of the same run
            out = {"kernel": r["kernel"], "pix_fmt": r["pix_fmt"], "calls": r["calls"], "us_per_4k_frame": round(r["us"], 2)}
            if r["pix_fmt"] in sdr and resize_us is not None:
                chain = sdr[r["pix_fmt"]] + resize_us
                out.update(chain_decode_us=round(sdr[r["pix_fmt"]], 2), chain_resize_us=round(resize_us, 2), chain_us_per_4k_frame=round(chain, 2),
                           chain_over_fused=round(chain / r["us"], 2))
            print(json.dumps(out))
            continue
        if r["transfer"] is not None and args.transfer and r["transfer"] not in args.transfer:
            continue
        if r["kernel"] in scaled_hdr:  # beside the HDR decode kernel of the same format and transfer + the resize kernel of the same run
            out = {"kernel": r["kernel"], "pix_fmt": r["pix_fmt"], "transfer": r["transfer"], "calls": r["calls"], "us_per_4k_frame": round(r["us"], 2)}
            if args.scale:  # the bytes the fused kernel moves: the payload in, 3 B per destination pixel out (p010le at 2 x 2: 3.75 B/px)
                nbytes = frame_size(r["pix_fmt"], H, W) + 3.0 * args.scale[0] * args.scale[1]
                out.update(bytes_per_src_px=round(nbytes / (H * W), 3), **{"frac_of_6.29TBps": round(nbytes / COPY_BPS / (r["us"] * 1e-6), 3)})
            key = (r["pix_fmt"], r["transfer"])
            if key in hdr_us and resize_us is not None:
                chain = hdr_us[key] + resize_us
                out.update(chain_decode_us=round(hdr_us[key], 2), chain_resize_us=round(resize_us, 2), chain_us_per_4k_frame=round(chain, 2),
                           chain_over_fused=round(chain / r["us"], 2))
            print(json.dumps(out))
            continue
        fmt, us = "yuv420p" if r["pix_fmt"] == "i420" else r["pix_fmt"], r["us"]
        bytes_per_frame = frame_size(fmt, H, W) + 3.0 * H * W  # the payload + 3 B/px of RGB, in one direction
        out = {"kernel": r["kernel"], "pix_fmt": r["pix_fmt"], "calls": r["calls"], "us_per_4k_frame": round(us, 2),
               "TB_per_s": round(bytes_per_frame / (us * 1e-6) / 1e12, 3), "frac_of_6.29TBps": round(bytes_per_frame / COPY_BPS / (us * 1e-6), 3)}
        if r["transfer"] is not None:
            out["transfer"] = r["transfer"]
            if r["pix_fmt"] in sdr:
                out["x_sdr_decode"] = round(us / sdr[r["pix_fmt"]], 2)
        print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("stream")
    s.add_argument("--frames", type=int, default=256)
    s.add_argument("--distinct", type=int, default=32)
    s.add_argument("--reps", type=int, default=3)
    s.add_argument("--pix-fmt", nargs="+", default=None, help="raw formats to stream with io_format='yuv' (the baseline is io_format='i420')")
    k = sub.add_parser("kernels")
    k.add_argument("--iters", type=int, default=20)
    k.add_argument("--pix-fmt", nargs="+", default=None, help="raw formats to run through the avx_yuv_to_rgb_u8 / avx_rgb_to_yuv_u8 kernels too")
    k.add_argument("--transfer", nargs="+", default=None, choices=["pq", "hlg"], help="also run the HDR decode of every named 10-bit format with these transfers")
    k.add_argument("--scale", default=None, type=lambda t: tuple(int(v) for v in t.lower().split("x")), metavar="WxH",
                   help="also run the scaled decode of every named format to this size, beside avx_yuv_to_rgb_u8 + avx_resize_hwc per frame")
    r = sub.add_parser("report")
    r.add_argument("csv")
    r.add_argument("--transfer", nargs="+", default=None, choices=["pq", "hlg"], help="keep only these transfers' HDR kernels")
    r.add_argument("--scale", default=None, type=lambda t: tuple(int(v) for v in t.lower().split("x")), metavar="WxH",
                   help="the --scale of the run: a scaled HDR decode kernel's line then carries its share of the copy rate")
    args = ap.parse_args()
    {"stream": stream, "kernels": kernels, "report": report}[args.cmd](args)


if __name__ == "__main__":
    main()
