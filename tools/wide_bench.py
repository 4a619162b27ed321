"""The wide view of the dichromats: the two routes behind avx_dichromat_wide_u8 against the chain that defines them and
against the species' plain day kernel.  Not part of bench.py.

  python tools/wide_bench.py [--reps 7] [--only 1080p] [--species Dog Rat] [--tiles] [--out FILE]

Batches of eight device-resident frames at 1080p and 4K for Dog (r = 14), Lion (r = 5), Rat (row gain) and Horse (streak), Cat's
geometry (105:40, camera 100).  Forms, interleaved repetition by repetition in one process, every repetition between its own pair of
events on the stream:
  chain        avx_binocular_warp_u8 per frame into float32 frames, then avx_dichromat_u8(in_f32 = 1) on the batch -- the entry points
               of the parent commit (not Horse: the streak species have no chain)
  wide_fused   avx_dichromat_wide_u8 under AVX_WIDE_ROUTE=fused (not Horse)
  wide_planes  avx_dichromat_wide_u8 under AVX_WIDE_ROUTE=planes
  wide         avx_dichromat_wide_u8 as the entry routes it by default
  day          avx_dichromat_u8 on the uint8 frames: the species without the wide view
One JSON line per (species, size, form): median and min-max in microseconds per frame.  --tiles adds the fused kernel's tile table
(AVX_WIDE_TILE) at r = 0, 3, 8 and 14 (Rat, Squirrel, Raccoon, Dog) at 1080p."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIZES = [("1080p", 1080, 1920), ("4k", 2160, 3840)]
SPECIES = ["Dog", "Lion", "Rat", "Horse"]
TILE_SPECIES = ["Rat", "Squirrel", "Raccoon", "Dog"]
TILES = ["32x8", "32x16", "32x32", "64x16", "64x32", "64x64", "128x16", "128x32"]
GEOMETRY = (105.0, 40.0, 100.0)  # phi, O, camera: Cat's
BATCH = 8


def _pool(n, H, W):
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    return np.stack([structured_frame(k, H, W) if k % 2 else noise_frame(k, H, W) for k in range(n)])


def _with_env(run, **env):
    """run() with the library's switches set for this call (it reads them per call) and removed again."""
    def wrapped():
        for k, v in env.items():
            os.environ[k] = v
        try:
            run()
        finally:
            for k in env:
                del os.environ[k]

    return wrapped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="repetitions per form (default 7)")
    ap.add_argument("--only", nargs="*", default=None, help="1080p and / or 4k")
    ap.add_argument("--species", nargs="*", default=None, choices=SPECIES + ["Squirrel", "Raccoon"])
    ap.add_argument("--tiles", action="store_true", help="also the fused kernel's tile table at r = 0, 3, 8, 14 (1080p)")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("wide_bench: at least five repetitions per form")
    from animal_vision_amd import animals
    from animal_vision_amd import geometry as G
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.runtime import device_count, get_context

    if device_count() < 1:
        raise SystemExit("wide_bench: needs a GPU (there is no CPU path to time)")
    ctx = get_context()
    out = open(args.out, "w") if args.out else None
    phi, overlap, camera = GEOMETRY

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def measure(forms, s, tag):
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
            emit({"bench": "wide", **tag, "form": k, "batch": BATCH, "reps": len(us), "us_per_frame_median": round(med[k], 1),
                  "us_per_frame_min": round(us[0], 1), "us_per_frame_max": round(us[-1], 1)})
        return med

    for size, H, W in SIZES:
        if args.only and size not in args.only:
            continue
        frames = _pool(BATCH, H, W)
        host_tables = G.binocular_warp_tables(H, W, W, H, camera, phi, overlap)
        s = ctx.stream_create()
        d_in, d_out, d_f32 = ctx.upload(frames, stream=s), ctx.malloc(frames.nbytes), ctx.malloc(frames.nbytes * 4)
        tab, ptrs = G.binocular_warp_tables_device(ctx, host_tables)
        fb = H * W * 3
        try:
            names = list(args.species or SPECIES) + (TILE_SPECIES if args.tiles and size == "1080p" else [])
            for i, name in enumerate(names):
                spec = getattr(animals, name).SPEC
                tiles = i >= len(args.species or SPECIES)
                op, op_f32 = DichromatOp(spec, ctx), DichromatOp(spec, ctx)
                op.prepare_tables(H)
                op_f32.desc.in_f32 = 1

                def wide(op=op):
                    G.dichromat_wide_device(ctx, d_in, d_out, BATCH, H, W, op.desc, ptrs, stream=s)

                def chain(op_f32=op_f32):
                    for f in range(BATCH):
                        G.binocular_warp_device(ctx, d_in.view(f * fb, fb), H, W, host_tables, H, W, d_f32.view(f * fb * 4, fb * 4), stream=s)
                    op_f32.run_device(d_f32, d_out, BATCH, H, W, stream=s)

                if tiles:
                    forms = {t: _with_env(wide, AVX_WIDE_ROUTE="fused", AVX_WIDE_TILE=t) for t in TILES}
                    measure(forms, s, {"species": name, "size": size, "table": "tiles", "r": op.desc.ksize // 2})
                    continue
                forms = {}
                if spec.post != "streak":
                    forms["chain"] = chain
                    forms["wide_fused"] = _with_env(wide, AVX_WIDE_ROUTE="fused")
                forms["wide_planes"] = _with_env(wide, AVX_WIDE_ROUTE="planes")
                forms["wide"] = wide
                forms["day"] = lambda op=op: op.run_device(d_in, d_out, BATCH, H, W, stream=s)
                med = measure(forms, s, {"species": name, "size": size})
                emit({"bench": "wide", "species": name, "size": size, **{f"{k}_over_day": round(v / med["day"], 2) for k, v in med.items() if k != "day"}})
        finally:
            ctx.sync(s)
            for b in (d_in, d_out, d_f32, tab):
                b.free()
            ctx.stream_destroy(s)


if __name__ == "__main__":
    main()
