"""The per-frame day/night switch against the plain day and night entries.  Not part of bench.py.

  python tools/daynight_bench.py [--reps 7] [--only 1080p] [--species Dog Rat] [--out FILE]

Batches of eight device-resident frames at 1080p and 4K.  Per species five forms, interleaved repetition by repetition in one process:
the day entry on a day batch, the night entry on a night batch, and the switched entry (avx_dichromat_auto_u8) on the all-day
batch, the all-night batch and a batch that alternates day and night frames (eight runs of one frame).  Every repetition is timed
twice at once: by a pair of events recorded on the stream around it, and by the host clock from before the call to after a
synchronisation of the stream -- the switched entry waits for its records inside the call, so its cost is host time, which the events
alone would not show for the forms that do not wait.  The decision kernel alone (avx_luma_mode_u8: the records' initialisation and the
one pass) is timed the same way, against the bytes it must read: 3 B per pixel at the 6.29 TB/s copy rate.
One JSON line per (species, size, form): median and min-max in microseconds per frame by both clocks; one more per (species, size)
with the overhead of the switched entry over the matching plain entry, by the host clock."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIZES = [("1080p", 1080, 1920), ("4k", 2160, 3840)]
SPECIES = ["Dog", "Lion", "Rat"]
BATCH = 8
COPY_RATE = 6.29e12  # B/s


def _pool(n, H, W, night):
    """n frames with content, day (codes 64..255) or night (codes 0..47) by a wide margin at the threshold 0.12."""
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    out = []
    for k in range(n):
        f = (structured_frame(k, H, W) if k % 2 else noise_frame(k, H, W)).astype(np.uint16)
        out.append((f * 47 // 255 if night else 64 + f * 191 // 255).astype(np.uint8))
    return np.stack(out)


def _stat(us):
    us = sorted(us)
    return {"median": round(statistics.median(us), 1), "min": round(us[0], 1), "max": round(us[-1], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="repetitions per form (default 7)")
    ap.add_argument("--only", nargs="*", default=None, help="1080p and / or 4k")
    ap.add_argument("--species", nargs="*", default=None, choices=SPECIES)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("daynight_bench: at least five repetitions per form")
    from animal_vision_amd import animals
    from animal_vision_amd._lib import LUMA_MODE_REC_DTYPE, lib
    from animal_vision_amd.dichromat import AutoNight, DichromatOp, NightSpec, luma_records_device
    from animal_vision_amd.runtime import device_count, get_context

    if device_count() < 1:
        raise SystemExit("daynight_bench: needs a GPU (there is no CPU path to time)")
    ctx = get_context()
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def measure(forms, s, warm=3):
        for run in forms.values():  # warm-up: code objects, workspaces, the day kernel's launch tuning, the clock ramp
            for _ in range(warm):
                run()
        ctx.sync(s)
        dev, host = {k: [] for k in forms}, {k: [] for k in forms}
        for _ in range(args.reps):
            for k, run in forms.items():
                t0 = time.perf_counter()
                ctx.timer_start(s)
                run()
                ms = ctx.timer_stop(s)  # (waits for the second event: the stream is idle again)
                host[k].append((time.perf_counter() - t0) * 1e6 / BATCH)
                dev[k].append(ms * 1e3 / BATCH)
        return dev, host

    for size, H, W in SIZES:
        if args.only and size not in args.only:
            continue
        day, night = _pool(BATCH, H, W, False), _pool(BATCH, H, W, True)
        mixed = np.stack([(night if k % 2 else day)[k] for k in range(BATCH)])
        s = ctx.stream_create()
        bufs = {k: ctx.upload(v, stream=s) for k, v in (("day", day), ("night", night), ("mixed", mixed))}
        d_out, d_rec = ctx.malloc(day.nbytes), ctx.malloc(16 * 16)
        rec_host = ctx.pinned((16,), LUMA_MODE_REC_DTYPE)
        try:
            # ---- the decision kernel alone, and with the copy of its records and the synchronisation the switch pays for
            forms = {
                "decision_kernel": lambda: ctx._check(lib.avx_luma_mode_u8(ctx._h, bufs["mixed"].ptr, BATCH, H, W, 0.12, d_rec.ptr, s)),
                "decision_with_records": lambda: luma_records_device(ctx, bufs["mixed"].ptr, BATCH, H, W, 0.12, d_rec, out=rec_host.array, stream=s),
            }
            dev, host = measure(forms, s)
            floor = 3.0 * H * W / COPY_RATE * 1e6
            for k in forms:
                emit({"bench": "daynight", "size": size, "form": k, "batch": BATCH, "reps": args.reps, "us_per_frame_events": _stat(dev[k]),
                      "us_per_frame_host": _stat(host[k]), "us_per_frame_bytes_at_copy_rate": round(floor, 2),
                      "events_median_over_bytes": round(statistics.median(dev[k]) / floor, 2)})
            modes = (rec_host.array["below"][:BATCH].astype(np.int64) * 2 > H * W).astype(int).tolist()
            assert modes == [k % 2 for k in range(BATCH)], modes  # the alternating batch alternates
            for name in args.species or SPECIES:
                spec = getattr(animals, name).SPEC
                ops = {"day": DichromatOp(spec, ctx), "night": DichromatOp(spec, ctx, night=NightSpec()), "auto": DichromatOp(spec, ctx, night=AutoNight())}
                forms = {
                    "day": lambda: ops["day"].run_device(bufs["day"], d_out, BATCH, H, W, stream=s),
                    "night": lambda: ops["night"].run_device(bufs["night"], d_out, BATCH, H, W, stream=s),
                    "auto_all_day": lambda: ops["auto"].run_device(bufs["day"], d_out, BATCH, H, W, stream=s),
                    "auto_all_night": lambda: ops["auto"].run_device(bufs["night"], d_out, BATCH, H, W, stream=s),
                    "auto_alternating": lambda: ops["auto"].run_device(bufs["mixed"], d_out, BATCH, H, W, stream=s),
                }
                dev, host = measure(forms, s)
                for k in forms:
                    emit({"bench": "daynight", "species": name, "size": size, "form": k, "batch": BATCH, "reps": args.reps,
                          "us_per_frame_events": _stat(dev[k]), "us_per_frame_host": _stat(host[k])})
                med = {k: statistics.median(v) for k, v in host.items()}
                emit({"bench": "daynight", "species": name, "size": size, "clock": "host",
                      "auto_all_day_minus_day_us_per_frame": round(med["auto_all_day"] - med["day"], 1),
                      "auto_all_night_minus_night_us_per_frame": round(med["auto_all_night"] - med["night"], 1),
                      "auto_alternating_minus_mean_of_day_and_night_us_per_frame": round(med["auto_alternating"] - 0.5 * (med["day"] + med["night"]), 1)})
        finally:
            ctx.sync(s)
            for b in list(bufs.values()) + [d_out, d_rec, rec_host]:
                b.free()
            ctx.stream_destroy(s)


if __name__ == "__main__":
    main()
