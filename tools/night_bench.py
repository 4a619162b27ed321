"""The night route of the dichromats against the day kernel of the same species.  Not part of bench.py.

  python tools/night_bench.py [--reps 7] [--only 1080p] [--species Dog Rat] [--out FILE]

Batches of eight device-resident frames at 1080p and 4K for Dog, Lion, Sheep, Rat and Cat: the day kernel (avx_dichromat_u8; Cat:
avx_cat_wide_u8), the night route without bloom and with bloom 0.12 (avx_dichromat_night_u8; Cat: avx_binocular_warp_u8 per frame into
float32 frames, then the night entry with in_f32 = 1), interleaved repetition by repetition in one process.  Every repetition is timed
by a pair of events recorded on the stream around it.  One JSON line per (species, size, form): median and min-max in microseconds per
frame; one more per (species, size) with night / day from that run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIZES = [("1080p", 1080, 1920), ("4k", 2160, 3840)]
SPECIES = ["Dog", "Lion", "Sheep", "Rat", "Cat"]
BATCH = 8
BLOOM = 0.12


def _pool(n, H, W):
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    return np.stack([structured_frame(k, H, W) if k % 2 else noise_frame(k, H, W) for k in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="repetitions per form (default 7)")
    ap.add_argument("--only", nargs="*", default=None, help="1080p and / or 4k")
    ap.add_argument("--species", nargs="*", default=None, choices=SPECIES)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("night_bench: at least five repetitions per form")
    from animal_vision_amd import animals
    from animal_vision_amd.animals._dichromats import CatStreamOp
    from animal_vision_amd.dichromat import DichromatOp, NightSpec
    from animal_vision_amd.runtime import device_count, get_context

    if device_count() < 1:
        raise SystemExit("night_bench: needs a GPU (there is no CPU path to time)")
    ctx = get_context()
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for size, H, W in SIZES:
        if args.only and size not in args.only:
            continue
        frames = _pool(BATCH, H, W)
        for name in args.species or SPECIES:
            cls = getattr(animals, name)
            s = ctx.stream_create()
            forms, closers = {}, []
            if name == "Cat":  # the stream operators: the slot's buffers, the warp tables (day: on the device; night: the chain's)
                for key, night in (("day", None), ("night", NightSpec()), ("night_bloom", NightSpec(bloom=BLOOM))):
                    sop = CatStreamOp(cls(night=night), H, W, depth=1, batch=BATCH, ctx=ctx)
                    sop.rect = None  # the wide view alone: the baseline launch is the same by day and by night
                    d_in, d_out = sop.slot_buffers(0)
                    ctx.upload(frames, d_in, stream=s)
                    forms[key] = lambda sop=sop, d_in=d_in, d_out=d_out: sop.run_device(d_in, d_out, BATCH, H, W, stream=s)
                    closers.append(sop.close)
            else:
                d_in, d_out = ctx.upload(frames, stream=s), ctx.malloc(frames.nbytes)
                closers += [d_in.free, d_out.free]
                for key, night in (("day", None), ("night", NightSpec()), ("night_bloom", NightSpec(bloom=BLOOM))):
                    op = DichromatOp(cls.SPEC, ctx, night=night)
                    forms[key] = lambda op=op: op.run_device(d_in, d_out, BATCH, H, W, stream=s)
            try:
                for run in forms.values():  # warm-up: code objects, workspaces, the day kernel's launch tuning, the clock ramp
                    for _ in range(3):
                        run()
                ctx.sync(s)
                times = {k: [] for k in forms}
                for _ in range(args.reps):
                    for k, run in forms.items():
                        ctx.timer_start(s)
                        run()
                        times[k].append(ctx.timer_stop(s) * 1e3 / BATCH)  # ms per batch -> us per frame
                med = {}
                for k, us in times.items():
                    us = sorted(us)
                    med[k] = statistics.median(us)
                    emit({"bench": "night", "species": name, "size": size, "form": k, "batch": BATCH, "reps": len(us),
                          "us_per_frame_median": round(med[k], 1), "us_per_frame_min": round(us[0], 1), "us_per_frame_max": round(us[-1], 1)})
                emit({"bench": "night", "species": name, "size": size, **{f"{k}_over_day": round(v / med["day"], 2) for k, v in med.items() if k != "day"}})
            finally:
                ctx.sync(s)
                for close in closers:
                    close()
                ctx.stream_destroy(s)


if __name__ == "__main__":
    main()
