"""Frames batched through the plane-program UV species against the four-lane form.  Not part of bench.py.

  python tools/uv_batch_bench.py [--reps 7] [--frames 96] [--only hummingbird_1080p] [--out FILE]

Device-resident (the frames are uploaded once), one process, the three forms of a workload interleaved rep by rep after a warm-up
pass of each, a host clock around work that ends in a device synchronise:

  lanes4   four single-frame plans on four streams forked from / joined into one (what bench.py's UV legs run)
  batch4   one plan with frames=4 on one stream
  batch8   one plan with frames=8 on one stream

Every form pushes the same `--frames` frames per timed window.  One JSON line per (workload, form): median, min and max over the
reps of microseconds per frame and MP/s, and, per workload, the ratio of the medians.  `kseq` runs form batch8 alone, for
`rocprofv3 --kernel-trace --stats -- python tools/uv_batch_bench.py kseq` (launches per batch)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WORKLOADS = [("hummingbird_1080p", "hummingbird", 1080, 1920), ("reindeer_1080p", "reindeer", 1080, 1920), ("kestrel_1080p", "kestrel", 1080, 1920),
             ("hummingbird_4k", "hummingbird", 2160, 3840)]


def _forms(ctx, sp, H, W, which):
    """name -> (run(frames), close): each enqueues `frames` frames and returns without synchronising."""
    from animal_vision_amd.animals._uv_species import SpeciesStreamOp
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    pool = np.stack([structured_frame(k, H, W) if k % 2 else noise_frame(k, H, W) for k in range(8)])
    forms = {}
    if "lanes4" in which:
        sop = SpeciesStreamOp(sp, H, W, depth=4, ctx=ctx)
        for k, be in enumerate(sop.plans):
            ctx.upload(pool[k], be.d_in)
        main, lanes = ctx.stream_create(), [ctx.stream_create() for _ in range(4)]

        def run_lanes(frames, sop=sop, main=main, lanes=lanes):
            for ls in lanes:
                ctx.stream_wait(ls, main)
            for j in range(frames):
                sop.plans[j % 4].run_device(lanes[j % 4])
            for ls in lanes:
                ctx.stream_wait(main, ls)
            return main

        def close_lanes(sop=sop, main=main, lanes=lanes):
            sop.close()
            for s in [main] + lanes:
                ctx.stream_destroy(s)

        forms["lanes4"] = (run_lanes, close_lanes)
    for n in (4, 8):
        if f"batch{n}" not in which:
            continue
        sop = SpeciesStreamOp(sp, H, W, depth=1, ctx=ctx, batch=n)
        ctx.upload(pool[:n], sop.plans[0].d_in)
        s = ctx.stream_create()

        def run_batch(frames, sop=sop, s=s, n=n):
            for _ in range(frames // n):
                sop.plans[0].run_device(s, n)
            return s

        def close_batch(sop=sop, s=s):
            sop.close()
            ctx.stream_destroy(s)

        forms[f"batch{n}"] = (run_batch, close_batch)
    return forms


def bench(args):
    from animal_vision_amd import animals
    from animal_vision_amd.runtime import device_count, get_context

    if device_count() < 1:
        raise SystemExit("uv_batch_bench: needs a GPU (there is no CPU path to time)")
    ctx = get_context()
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    assert args.frames % 8 == 0
    for name, mod, H, W in WORKLOADS:
        if args.only and name not in args.only:
            continue
        sp = getattr(animals, animals.UV_CLASS[mod])()
        frames = args.frames if H < 2000 else max(8, args.frames // 2)
        forms = _forms(ctx, sp, H, W, ("lanes4", "batch4", "batch8"))
        times = {k: [] for k in forms}
        for k, (run, _) in forms.items():  # warm-up: code objects, workspaces, the clock ramp
            for _ in range(2):
                ctx.sync(run(frames))
        for _ in range(args.reps):
            for k, (run, _) in forms.items():
                ctx.device_sync()
                t0 = time.perf_counter()
                ctx.sync(run(frames))
                times[k].append((time.perf_counter() - t0) / frames)
        med = {}
        for k, ts in times.items():
            us = sorted(t * 1e6 for t in ts)
            med[k] = statistics.median(us)
            mp = H * W / 1e6
            emit({"workload": name, "form": k, "frames_per_window": frames, "reps": len(us), "us_per_frame_median": round(med[k], 1),
                  "us_per_frame_min": round(us[0], 1), "us_per_frame_max": round(us[-1], 1), "MPps_median": round(mp / med[k] * 1e6, 0),
                  "MPps_min": round(mp / us[-1] * 1e6, 0), "MPps_max": round(mp / us[0] * 1e6, 0)})
        emit({"workload": name, "batch4_over_lanes4": round(med["lanes4"] / med["batch4"], 3), "batch8_over_lanes4": round(med["lanes4"] / med["batch8"], 3)})
        for _, close in forms.values():
            close()
    if out:
        out.close()


def kseq(args):
    """Form batch8 of hummingbird 1080p alone: 2 warm-up replays, then `--batches` replays (8 frames each) for the kernel trace."""
    from animal_vision_amd import animals
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    run, close = _forms(ctx, animals.Hummingbird(), 1080, 1920, ("batch8",))["batch8"]
    ctx.sync(run(8 * (2 + args.batches)))
    print(json.dumps({"kseq": "hummingbird_1080p batch8", "replays": 2 + args.batches, "frames_per_replay": 8}))
    close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", nargs="?", default="bench", choices=["bench", "kseq"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=96, help="frames per timed window (a multiple of 8; halved at 4K)")
    ap.add_argument("--only", nargs="*", default=None, help="workload names")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    ap.add_argument("--batches", type=int, default=10)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("uv_batch_bench: at least five repetitions per form")
    {"bench": bench, "kseq": kseq}[args.cmd](args)


if __name__ == "__main__":
    main()
