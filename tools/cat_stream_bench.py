"""Cat's fused wide-view kernel and stream against what they replace.  Not part of bench.py.

  python tools/cat_stream_bench.py kernels [--reps 9] [--tiles 32x24 32x32 ...] [--only 1080p] [--out FILE]
  python tools/cat_stream_bench.py stream  [--reps 5] [--frames 48] [--only 1080p] [--out FILE]

kernels  batches of eight device-resident frames at 1080p and 4K through avx_cat_wide_u8 and, in the same process and interleaved
         rep by rep, through the chain it replaces (avx_binocular_warp_u8 + avx_dichromat_u8(in_f32) frame by frame, the float32
         frame in between).  Every repetition is timed by a pair of events recorded on the stream around it.  One JSON line per
         (size, form): median and min-max in microseconds per frame, and chain / fused.  --tiles times the fused kernel at other
         output tiles too (AVX_CAT_TILE, a tuning switch of the library), each as a form of its own in the same interleaving.
stream   the Cat stream with split-compare from frames held in memory: FramePipeline(CatStreamOp) at batch 1 and 8, and the
         per-frame loop the video command ran for Cat before it streamed (visualize() as it then was -- zoom through a resize
         of its own, three allocations, the warp with its host tables, the float32 frame, the reference kernel -- and
         split_compose on the host), restated here.  Frames per second of each, median and min-max over the repetitions."""
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
BATCH = 8


def _pool(n, H, W):
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    return np.stack([structured_frame(k, H, W) if k % 2 else noise_frame(k, H, W) for k in range(n)])


def _emitter(path):
    out = open(path, "w") if path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    return emit


def _need_gpu():
    from animal_vision_amd.runtime import device_count, get_context

    if device_count() < 1:
        raise SystemExit("cat_stream_bench: needs a GPU (there is no CPU path to time)")
    return get_context()


def kernels(args):
    from animal_vision_amd import geometry as G
    from animal_vision_amd.animals import Cat
    from animal_vision_amd.dichromat import DichromatOp

    ctx = _need_gpu()
    emit = _emitter(args.out)
    cat = Cat()
    for name, H, W in SIZES:
        if args.only and name not in args.only:
            continue
        frames = _pool(BATCH, H, W)
        fbytes = H * W * 3
        op = DichromatOp(cat.SPEC, ctx)
        op_f32 = DichromatOp(cat.SPEC, ctx)
        op_f32.desc.in_f32 = 1
        tables = G.binocular_warp_tables(H, W, W, H, cat.CAMERA_HFOV_DEG, cat.CAT_PER_EYE_HALF_FOV_DEG, cat.CAT_OVERLAP_DEG)
        d_tab, ptrs = G.binocular_warp_tables_device(ctx, tables)
        d_in, d_out, d_ref, d_warp = ctx.upload(frames), ctx.malloc(frames.nbytes), ctx.malloc(frames.nbytes), ctx.malloc(fbytes * 4)
        s = ctx.stream_create()

        def chain():
            for f in range(BATCH):
                G.binocular_warp_device(ctx, d_in.view(f * fbytes, fbytes), H, W, tables, H, W, d_warp, s)
                op_f32.run_device(d_warp, d_ref.view(f * fbytes, fbytes), 1, H, W, stream=s)

        def fused(tile):
            def run():
                if tile:
                    os.environ["AVX_CAT_TILE"] = tile
                else:
                    os.environ.pop("AVX_CAT_TILE", None)
                G.cat_wide_device(ctx, d_in, d_out, BATCH, H, W, op.desc, ptrs, s)

            return run

        forms = {"chain": chain, "fused": fused(None)}
        for t in args.tiles or []:
            forms[f"fused_{t}"] = fused(t)
        try:
            want = None
            for k, run in forms.items():  # warm-up: code objects, workspaces, the clock ramp; the forms write the same bytes
                for _ in range(3):
                    run()
                got = ctx.download(d_ref if k == "chain" else d_out, frames.shape, np.uint8, stream=s)
                want = got if want is None else want
                if not np.array_equal(got, want):
                    raise SystemExit(f"cat_stream_bench: {k} at {name} differs from the chain")
                ctx.memset(d_out, 0, stream=s)
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
                emit({"bench": "kernels", "size": name, "form": k, "batch": BATCH, "reps": len(us), "us_per_frame_median": round(med[k], 1),
                      "us_per_frame_min": round(us[0], 1), "us_per_frame_max": round(us[-1], 1)})
            emit({"bench": "kernels", "size": name, **{f"chain_over_{k}": round(med["chain"] / v, 2) for k, v in med.items() if k != "chain"}})
        finally:
            os.environ.pop("AVX_CAT_TILE", None)
            ctx.sync(s)
            ctx.stream_destroy(s)
            for b in (d_tab, d_in, d_out, d_ref, d_warp):
                b.free()


def _per_frame_loop(ctx, cat, op, frames, labels):
    """The loop video.main ran for Cat before it had a stream operator, with visualize() as it was then."""
    from animal_vision_amd import geometry as G
    from animal_vision_amd.renderers import split_compose

    n = 0
    for image in frames:
        H, W = image.shape[:2]
        scale = G.zoom_scale_from_cat_ratio(camera_hfov_deg=cat.CAMERA_HFOV_DEG, cat_per_eye_half_fov_deg=cat.CAT_PER_EYE_HALF_FOV_DEG,
                                            cat_to_human_ratio=cat.CAT_TO_HUMAN_RATIO)
        human_zoomed = G.center_zoom(image, scale=scale)
        tables = G.binocular_warp_tables(H, W, W, H, cat.CAMERA_HFOV_DEG, cat.CAT_PER_EYE_HALF_FOV_DEG, cat.CAT_OVERLAP_DEG)
        d_in = ctx.upload(image)
        d_warp = ctx.malloc(H * W * 3 * 4)
        d_out = ctx.malloc(H * W * 3)
        try:
            G.binocular_warp_device(ctx, d_in, H, W, tables, H, W, d_warp)
            op.desc.in_f32 = 1
            try:
                op.run_device(d_warp, d_out, 1, H, W)
            finally:
                op.desc.in_f32 = 0
            cat_out = ctx.download(d_out, image.shape, np.uint8)
        finally:
            d_in.free(); d_warp.free(); d_out.free()
        split_compose(human_zoomed, cat_out, left_label=labels[0], right_label=labels[1])
        n += 1
    return n


def stream(args):
    from animal_vision_amd.animals import Cat
    from animal_vision_amd.animals._dichromats import CatStreamOp
    from animal_vision_amd.dichromat import DichromatOp
    from animal_vision_amd.pipeline import FramePipeline

    ctx = _need_gpu()
    emit = _emitter(args.out)
    cat = Cat()
    labels = ("Original", "Transformed")
    for name, H, W in SIZES:
        if args.only and name not in args.only:
            continue
        nframes = args.frames if H < 2000 else max(BATCH, args.frames // 2)
        pool = _pool(8, H, W)
        frames = [pool[k % 8] for k in range(nframes)]
        forms = {}
        ops = []
        for batch in (1, BATCH):
            op = CatStreamOp(cat, H, W, depth=3, batch=batch, ctx=ctx)
            pipe = FramePipeline(op, H, W, ctx=ctx, depth=3, split_compare=True, labels=labels, split_baseline=True, batch=batch)
            ops.append((op, pipe))
            forms[f"stream_batch{batch}"] = lambda pipe=pipe: pipe.run(iter(enumerate(frames)), lambda i, o: None).frames
        loop_op = DichromatOp(cat.SPEC, ctx)
        forms["per_frame_loop"] = lambda: _per_frame_loop(ctx, cat, loop_op, frames[:max(4, nframes // 4)], labels)
        try:
            for run in forms.values():  # warm-up
                run()
            fps = {k: [] for k in forms}
            for _ in range(args.reps):
                for k, run in forms.items():
                    ctx.device_sync()
                    t0 = time.perf_counter()
                    n = run()
                    ctx.device_sync()
                    fps[k].append(n / (time.perf_counter() - t0))
            med = {}
            for k, v in fps.items():
                v = sorted(v)
                med[k] = statistics.median(v)
                emit({"bench": "stream", "size": name, "form": k, "reps": len(v), "fps_median": round(med[k], 1), "fps_min": round(v[0], 1),
                      "fps_max": round(v[-1], 1)})
            emit({"bench": "stream", "size": name, **{f"{k}_over_per_frame_loop": round(v / med["per_frame_loop"], 2) for k, v in med.items() if k != "per_frame_loop"}})
        finally:
            for op, pipe in ops:
                pipe.close()
                op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["kernels", "stream"])
    ap.add_argument("--reps", type=int, default=None, help="repetitions per form (default 9 for kernels, 5 for stream)")
    ap.add_argument("--frames", type=int, default=48, help="stream: frames per timed run (halved at 4K)")
    ap.add_argument("--tiles", nargs="*", default=None, metavar="WxH", help="kernels: also time the fused kernel at these output tiles")
    ap.add_argument("--only", nargs="*", default=None, help="1080p and / or 4k")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 9 if args.cmd == "kernels" else 5
    if args.reps < 5:
        raise SystemExit("cat_stream_bench: at least five repetitions per form")
    {"kernels": kernels, "stream": stream}[args.cmd](args)


if __name__ == "__main__":
    main()
