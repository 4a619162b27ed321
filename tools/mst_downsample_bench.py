"""HoneyBee on MST++ with the network at reduced resolution against the full-size network.  Not part of bench.py.

  timeout -k 10 600 python tools/mst_downsample_bench.py --only 4k --out 4k.jsonl && \\
  timeout -k 10 600 python tools/mst_downsample_bench.py --only 1080p --out 1080p.jsonl

(one size per process, each GPU step under its own time limit, the steps chained with &&).

Device-resident (the frame is uploaded once), one process, the forms of a size -- the full-size route and hsi_scale 0.5, 0.25 and 0.1 --
interleaved rep by rep after a warm-up pass of each, a host clock around work that ends in a device synchronise; seeded weights (the
arithmetic does not depend on them).  Per (size, form) one JSON line: median, min and max over the reps of milliseconds per frame and
frames per second, and the ratio of the full-size median to the form's.  Beside them:

  * `catch_planes_up`: avx_catch_planes_up alone between two stream events (`--kernel-launches` launches per window), with the bytes it
    reads and writes;
  * `difference`: mean absolute and maximum code difference of each reduced form's output from the full-size output on
    synthetic.structured_frame -- information on what the speed costs, not a pass mark."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIZES = [("4k", 2160, 3840), ("1080p", 1080, 1920)]
SCALES = [None, 0.5, 0.25, 0.1]


def _name(scale):
    return "full" if scale is None else f"hsi_scale_{scale:g}"


def bench(args):
    import torch

    from animal_vision_amd import animals
    from animal_vision_amd._lib import lib
    from animal_vision_amd.ml import MSTPlusPlusPredictor
    from animal_vision_amd.ml.predict import reduced_size
    from animal_vision_amd.runtime import DeviceBuffer, device_count
    from animal_vision_amd.synthetic import structured_frame

    if device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("mst_downsample_bench: needs a GPU (there is no CPU path to time)")
    pred = MSTPlusPlusPredictor(None, seed=0, half=True).prepare()
    op32 = animals.HoneyBee()._operator().padded_clone(32)
    ctx = op32._ctx()
    out = open(args.out, "w") if args.out else None
    rows = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name, H, W in SIZES:
        if args.only and name not in args.only:
            continue
        frames = args.frames if H < 2000 else max(4, args.frames // 2)
        t_in = torch.from_numpy(structured_frame(3, H, W)).to(pred.device)
        stream = ctx.stream_create()
        ext = torch.cuda.ExternalStream(stream, device=pred.device)
        forms = {}
        for scale in SCALES:
            small = reduced_size(H, W, scale, pred.stride)
            t_out = torch.empty((H, W, 3), dtype=torch.uint8, device=pred.device)
            forms[_name(scale)] = (scale, small, t_out, DeviceBuffer(ctx, t_out.data_ptr(), t_out.numel(), owned=False),
                                   pred.reduced_work(H, W, small) if small is not None else None)

        def run(form, n):
            scale, _, _, d_out, work = forms[form]
            with torch.cuda.stream(ext):
                for _ in range(n):
                    for tns in pred.honeybee_device(t_in, op32, d_out, stream, hsi_scale=scale, work=work):
                        tns.record_stream(ext)

        times = {k: [] for k in forms}
        for k in forms:  # warm-up: code objects, workspaces, resize tables, the allocator's pools, the clock ramp
            for _ in range(2):
                run(k, frames)
                ctx.sync(stream)
        for _ in range(args.reps):
            for k in forms:
                ctx.device_sync()
                t0 = time.perf_counter()
                run(k, frames)
                ctx.sync(stream)
                times[k].append((time.perf_counter() - t0) / frames)
        med = {k: statistics.median(ts) * 1e3 for k, ts in times.items()}
        full = forms["full"][2].cpu().numpy().astype(np.int16)
        for k, ts in times.items():
            ms = sorted(t * 1e3 for t in ts)
            small = forms[k][1]
            rec = {"size": name, "form": k, "network_hw": list(small) if small else [H, W], "frames_per_window": frames, "reps": len(ms),
                   "ms_per_frame_median": round(med[k], 3), "ms_per_frame_min": round(ms[0], 3), "ms_per_frame_max": round(ms[-1], 3),
                   "fps_median": round(1e3 / med[k], 1), "fps_min": round(1e3 / ms[-1], 1), "fps_max": round(1e3 / ms[0], 1),
                   "full_over_form": round(med["full"] / med[k], 2)}
            if small:
                d = np.abs(forms[k][2].cpu().numpy().astype(np.int16) - full)
                rec["difference"] = {"mean_abs_code": round(float(d.mean()), 3), "max_code": int(d.max())}
            emit(rec)
            rows.append(rec)
        # the new kernel alone, between stream events
        for k, (scale, small, _, _, work) in forms.items():
            if small is None:
                continue
            h, w = small
            src = torch.rand((3, h, w), dtype=torch.float32, device=pred.device)
            n = ctypes.c_int(0)

            def window():
                ctx.timer_start(stream)
                for _ in range(args.kernel_launches):
                    ctx._check(lib.avx_catch_planes_up(ctx._h, src.data_ptr(), h, w, work["planes"].data_ptr(), H, W, work["partials"].data_ptr(),
                                                       ctypes.byref(n), stream))
                return ctx.timer_stop(stream) * 1e3 / args.kernel_launches  # us per launch

            torch.cuda.synchronize(pred.device)
            window()
            us = sorted(window() for _ in range(args.reps))
            nbytes = 12 * H * W + 12 * h * w
            rec = {"size": name, "kernel": "catch_planes_up", "form": k, "from_hw": [h, w], "launches_per_window": args.kernel_launches, "reps": len(us),
                   "us_median": round(statistics.median(us), 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1), "bytes": nbytes,
                   "records": n.value, "GBps_median": round(nbytes / statistics.median(us) / 1e3, 0)}
            emit(rec)
            rows.append(rec)
        torch.cuda.synchronize(pred.device)
        del ext, forms
        torch.cuda.empty_cache()
        ctx.stream_destroy(stream)
    print("\n| size | form | network | ms / frame, median (min-max) | fps | full / form | mean abs / max code difference |\n|---|---|---|---|---|---|---|")
    for r in rows:
        if "kernel" not in r:
            d = r.get("difference")
            print(f"| {r['size']} | {r['form']} | {r['network_hw'][1]}x{r['network_hw'][0]} | {r['ms_per_frame_median']} ({r['ms_per_frame_min']}-"
                  f"{r['ms_per_frame_max']}) | {r['fps_median']} | {r['full_over_form']} | {'-' if d is None else str(d['mean_abs_code']) + ' / ' + str(d['max_code'])} |")
    print("\n| size | avx_catch_planes_up from | us, median (min-max) | bytes | GB/s | records |\n|---|---|---|---|---|---|")
    for r in rows:
        if "kernel" in r:
            print(f"| {r['size']} | {r['from_hw'][1]}x{r['from_hw'][0]} | {r['us_median']} ({r['us_min']}-{r['us_max']}) | {r['bytes']} | {r['GBps_median']} | {r['records']} |")
    if out:
        out.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=32, help="frames per timed window (halved at 4K)")
    ap.add_argument("--kernel-launches", type=int, default=50, help="avx_catch_planes_up launches per event window")
    ap.add_argument("--only", nargs="*", default=None, choices=[s[0] for s in SIZES], help="sizes")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("mst_downsample_bench: at least five repetitions per form")
    bench(args)


if __name__ == "__main__":
    main()
