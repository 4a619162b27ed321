"""Time of the frame-metrics kernel and of the compare command.  Not part of bench.py.

  python tools/metrics_bench.py kernel [--reps 7]
      avx_frame_metrics_u8 on frames resident on the device, 1080p and 4K, batches of 1 and 8, with and without SSIM: every
      repetition between its own pair of stream events (the record memset and the final-reduction launch included), after one warm-up
      call.  One JSON line per configuration: median (min-max) in us per frame, and what the 6 B/px both frames hold would take at
      6.29 TB/s (the measured HBM copy rate, MI355X).  The frames are noise against the same noise +-2 codes: most differences are 0,
      1 or 2, as between two renderings of one clip, which is also the worst case of the histogram's LDS atomics.
  python tools/metrics_bench.py planes [--reps 7]
      avx_plane_metrics on nv12 and p010le pairs resident on the device, 4K and 1080p, batches of 8, the histogram
      alone and with SSIM, interleaved in one process with the RGB route on the same payloads (yuv_to_rgb_device for both sides, then
      avx_frame_metrics_u8; at 10 bits the RGB route compares what is left after rounding to 8 bits): per repetition each of the four
      forms once, each between its own pair of stream events, after one warm-up call of each.  One JSON line per (format, size, ssim):
      median (min-max) of both routes in us per frame, their ratio, and what the payload bytes of both sides (2 x 1.5 B/px for nv12,
      2 x 3 B/px for p010le) would take at 6.29 TB/s.  The pairs are noise against the same noise +-2 codes in every plane.
  python tools/metrics_bench.py ms [--reps 7]
      avx_frame_metrics_ms_u8 (MS-SSIM over five scales) on RGB pairs resident on the device, 4K and 1080p, batches of
      8, interleaved in one process with avx_frame_metrics_u8(with_ssim = 1) on the same frames: per repetition each of the two once,
      each between its own pair of stream events, after one warm-up call of each.  One JSON line per size: median (min-max) of both
      in us per frame and their ratio.  The pairs are noise against the same noise +-2 codes.
  python tools/metrics_bench.py command [--frames 32] [--reps 3] [--dir DIR]
      Two 4K nv12 files of `frames` frames in DIR (default: /dev/shm when there is one, so they are read from memory) through
      python -m animal_vision_amd.compare's main(), --batch 8, with SSIM, without it and with --ms-ssim: frames per second of the
      whole command (read, upload, decode, compare, CSV), `reps` runs each after one warm-up run."""
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
    from animal_vision_amd.metrics import RECORD_BYTES, frame_metrics_launch
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    for name, (H, W) in SIZES.items():
        a, b = _pair(8, H, W)
        d_a, d_b, d_out = ctx.upload(a), ctx.upload(b), ctx.malloc(8 * RECORD_BYTES)
        for n in (1, 8):
            for ssim in (True, False):
                frame_metrics_launch(ctx, d_a, d_b, n, H, W, d_out, ssim=ssim)  # warm-up: the workspace is sized here
                ctx.sync()
                each = []
                for _ in range(args.reps):
                    ctx.timer_start()
                    frame_metrics_launch(ctx, d_a, d_b, n, H, W, d_out, ssim=ssim)
                    each.append(ctx.timer_stop() * 1e3 / n)
                floor = 6.0 * H * W / COPY_BPS * 1e6
                print(json.dumps({"size": name, "batch": n, "ssim": ssim, "reps": args.reps, "us_per_frame_median": round(float(np.median(each)), 1),
                                  "us_per_frame_min": round(min(each), 1), "us_per_frame_max": round(max(each), 1),
                                  "us_6B_per_px_at_6.29TBps": round(floor, 1), "x_copy_floor": round(float(np.median(each)) / floor, 1)}), flush=True)
        for d in (d_a, d_b, d_out):
            d.free()


def _plane_pair(fmt, n, H, W, seed=0):
    """n payload pairs of `fmt`: noise, and the same noise +-2 codes in every sample."""
    wide = fmt == "p010le"
    top, ns = (1023, H * W * 3 // 2) if wide else (255, H * W * 3 // 2)
    rng = np.random.default_rng(seed)
    a = rng.integers(0, top + 1, (n, ns), dtype=np.int16)
    b = np.clip(a + rng.integers(-2, 3, a.shape, dtype=np.int16), 0, top)
    if wide:
        return (a.astype("<u2") << 6).view(np.uint8).reshape(n, -1), (b.astype("<u2") << 6).view(np.uint8).reshape(n, -1)
    return a.astype(np.uint8), b.astype(np.uint8)


def planes(args):
    from animal_vision_amd.metrics import PLANE_RECORD_BYTES, RECORD_BYTES, frame_metrics_launch, plane_metrics_launch
    from animal_vision_amd.runtime import get_context
    from animal_vision_amd.yuv import yuv_to_rgb_device

    ctx, n = get_context(), 8
    for name, (H, W) in (("4k", SIZES["4k"]), ("1080p", SIZES["1080p"])):
        d_ra, d_rb = ctx.malloc(n * H * W * 3), ctx.malloc(n * H * W * 3)
        d_out, d_pout = ctx.malloc(n * RECORD_BYTES), ctx.malloc(n * PLANE_RECORD_BYTES)
        for fmt in ("nv12", "p010le"):
            a, b = _plane_pair(fmt, n, H, W)
            d_a, d_b = ctx.upload(a), ctx.upload(b)

            def plane_route(ssim):
                plane_metrics_launch(ctx, fmt, d_a, d_b, n, H, W, d_pout, ssim=ssim)

            def rgb_route(ssim):
                yuv_to_rgb_device(ctx, fmt, d_a, d_ra, n, H, W)
                yuv_to_rgb_device(ctx, fmt, d_b, d_rb, n, H, W)
                frame_metrics_launch(ctx, d_ra, d_rb, n, H, W, d_out, ssim=ssim)

            forms = [(route, ssim) for ssim in (False, True) for route in (plane_route, rgb_route)]
            times = {k: [] for k in range(len(forms))}
            for route, ssim in forms:  # warm-up: the workspace is sized here
                route(ssim)
            ctx.sync()
            for _ in range(args.reps):
                for k, (route, ssim) in enumerate(forms):
                    ctx.timer_start()
                    route(ssim)
                    times[k].append(ctx.timer_stop() * 1e3 / n)
            floor = a.shape[1] * 2 / COPY_BPS * 1e6
            for k in (0, 2):
                pl, rg = times[k], times[k + 1]
                print(json.dumps({"planes": fmt, "size": name, "batch": n, "ssim": forms[k][1], "reps": args.reps,
                                  "plane_us_per_frame_median": round(float(np.median(pl)), 1), "plane_us_min": round(min(pl), 1),
                                  "plane_us_max": round(max(pl), 1), "rgb_route_us_per_frame_median": round(float(np.median(rg)), 1),
                                  "rgb_route_us_min": round(min(rg), 1), "rgb_route_us_max": round(max(rg), 1),
                                  "rgb_over_plane": round(float(np.median(rg)) / float(np.median(pl)), 2),
                                  "us_payload_bytes_at_6.29TBps": round(floor, 1),
                                  "plane_x_copy_floor": round(float(np.median(pl)) / floor, 1)}), flush=True)
            d_a.free()
            d_b.free()
        for d in (d_ra, d_rb, d_out, d_pout):
            d.free()


def ms(args):
    from animal_vision_amd.metrics import MS_RECORD_BYTES, RECORD_BYTES, frame_metrics_launch, frame_metrics_ms_launch
    from animal_vision_amd.runtime import get_context

    ctx, n = get_context(), 8
    for name, (H, W) in (("4k", SIZES["4k"]), ("1080p", SIZES["1080p"])):
        a, b = _pair(n, H, W)
        d_a, d_b, d_out, d_ms = ctx.upload(a), ctx.upload(b), ctx.malloc(n * RECORD_BYTES), ctx.malloc(n * MS_RECORD_BYTES)

        def ms_route():
            frame_metrics_ms_launch(ctx, d_a, d_b, n, H, W, d_out, d_ms)

        def ssim_route():
            frame_metrics_launch(ctx, d_a, d_b, n, H, W, d_out, ssim=True)

        forms = [ms_route, ssim_route]
        times = [[], []]
        for route in forms:  # warm-up: the workspace is sized here
            route()
        ctx.sync()
        for _ in range(args.reps):
            for k, route in enumerate(forms):
                ctx.timer_start()
                route()
                times[k].append(ctx.timer_stop() * 1e3 / n)
        m, s = times
        print(json.dumps({"ms_ssim": True, "size": name, "batch": n, "reps": args.reps, "ms_us_per_frame_median": round(float(np.median(m)), 1),
                          "ms_us_min": round(min(m), 1), "ms_us_max": round(max(m), 1), "ssim_us_per_frame_median": round(float(np.median(s)), 1),
                          "ssim_us_min": round(min(s), 1), "ssim_us_max": round(max(s), 1),
                          "ms_over_ssim": round(float(np.median(m)) / float(np.median(s)), 2)}), flush=True)
        for d in (d_a, d_b, d_out, d_ms):
            d.free()


def command(args):
    from animal_vision_amd import compare
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
        argv = [os.path.join(d, "a.yuv"), os.path.join(d, "b.yuv"), "--pix-fmt", "nv12", "--size", f"{W}x{H}", "--batch", "8",
                "--csv", os.path.join(d, "out.csv")]
        for extra in ([], ["--no-ssim"], ["--ms-ssim"]):
            fps = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                with contextlib.redirect_stderr(io.StringIO()):
                    status = compare.main(argv + extra)
                dt = time.perf_counter() - t0
                assert status == 0, status
                if rep:  # the first run is the warm-up
                    fps.append(args.frames / dt)
            print(json.dumps({"command": "compare", "size": "4k", "pix_fmt": "nv12", "frames": args.frames, "batch": 8, "ssim": extra != ["--no-ssim"],
                              "ms_ssim": extra == ["--ms-ssim"],
                              "reps": args.reps, "fps_median": round(float(np.median(fps)), 1), "fps_min": round(min(fps), 1),
                              "fps_max": round(max(fps), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--reps", type=int, default=7)
    pl = sub.add_parser("planes")
    pl.add_argument("--reps", type=int, default=7)
    m = sub.add_parser("ms")
    m.add_argument("--reps", type=int, default=7)
    c = sub.add_parser("command")
    c.add_argument("--frames", type=int, default=32)
    c.add_argument("--reps", type=int, default=3)
    c.add_argument("--dir", default=None)
    args = ap.parse_args()
    {"kernel": kernel, "planes": planes, "ms": ms, "command": command}[args.cmd](args)


if __name__ == "__main__":
    main()
