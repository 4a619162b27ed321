"""The species wall's batched compose and stream against what they replace.  Not part of bench.py.

  python tools/wall_bench.py kernels [--reps 9] [--only 1080p] [--out FILE]
  python tools/wall_bench.py stream  [--reps 5] [--frames 48] [--only 1080p] [--out FILE]

kernels  batches of eight frames of 20 (the Non-UV sheet) and of 5 device-resident tiles at 1080p and 4K, tile heights 256 and
         270, through avx_wall_compose_u8 (one launch, a resident layout) and, in the same process and interleaved rep by rep,
         through eight avx_gallery_compose_u8 calls on the same tiles (the existing entry point: one launch per sheet, descriptors
         uploaded whenever a source pointer changes).  Every repetition is timed by a pair of events recorded on the stream around
         it.  One JSON line per (workload, form): median and min-max in microseconds per frame, and the bytes per second over the
         bytes a sheet must move (n_tiles * H * W * 3 read, Hc * Wc * 3 written).  The canvases of both forms are compared first.
stream   the wall of {Dog, Cat, HoneyBee, ReinDeer} with the original, fed from memory with I420 payloads: FramePipeline(WallStreamOp)
         at batch 1 and 8, against the four species streamed one after the other in the same process (the sum of their times: what
         running the `video` command once per species costs before any tiling).  Frames per second of each, median and min-max."""
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

SIZES = [("1080p", 1080, 1920), ("4k", 2160, 3840)]
BATCH = 8
WALL = ["Dog", "Cat", "HoneyBee", "ReinDeer"]


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
        raise SystemExit("wall_bench: needs a GPU (there is no CPU path to time)")
    return get_context()


def kernels(args):
    from animal_vision_amd._lib import GalleryTile, lib
    from animal_vision_amd.gallery import NON_UV_NAMES
    from animal_vision_amd.wall import WallLayout

    ctx = _need_gpu()
    emit = _emitter(args.out)
    bg = (ctypes.c_int * 3)(20, 20, 20)
    for name, H, W in SIZES:
        if args.only and name not in args.only:
            continue
        fbytes = H * W * 3
        pool = _pool(4, H, W)
        for n_tiles in (20, 5):
            # tile i, frame f: a distinct offset into a pool of frames, so that no two tiles of a sheet are the same bytes
            d_src, d_pool = ctx.malloc(n_tiles * BATCH * fbytes), ctx.upload(pool)
            for k in range(n_tiles * BATCH):
                ctx._check(lib.avx_memcpy_d2d(ctx._h, d_src.ptr + k * fbytes, d_pool.ptr + (k % 4) * fbytes, fbytes, ctx._s(None)))
            ctx.sync()
            d_pool.free()
            for tile_height in (256, 270):
                lay = WallLayout(NON_UV_NAMES[:n_tiles], H, W, tile_height, 8)
                Hc, Wc = lay.canvas_shape
                Hg, Wg = lay.grid_shape
                seg = np.ascontiguousarray(lay.segments, np.float32)
                segp = seg.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
                handle = ctypes.c_void_p()
                ctx._check(lib.avx_wall_layout_create(ctx._h, H, W, lay.h, lay.w, n_tiles, (ctypes.c_int * n_tiles)(*lay.seg_offsets),
                                                      (ctypes.c_int * n_tiles)(*lay.seg_counts), segp, len(seg), lay.strip_h, lay.pad, lay.cols, bg,
                                                      ctypes.byref(handle)))
                mode, staged, piece, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
                lib.avx_wall_layout_info(handle.value, ctypes.byref(mode), ctypes.byref(staged), ctypes.byref(piece), ctypes.byref(lds))
                d_wall, d_gal = ctx.malloc(BATCH * Hc * Wc * 3), ctx.malloc(BATCH * Hg * Wg * 3)
                srcs = (ctypes.c_void_p * n_tiles)(*(d_src.ptr + i * BATCH * fbytes for i in range(n_tiles)))
                descs = [(GalleryTile * n_tiles)(*(GalleryTile(d_src.ptr + (i * BATCH + f) * fbytes, 2, H, W, lay.h, lay.w, lay.seg_offsets[i],
                                                               lay.seg_counts[i]) for i in range(n_tiles))) for f in range(BATCH)]
                s = ctx.stream_create()

                def wall():
                    ctx._check(lib.avx_wall_compose_u8(ctx._h, handle.value, srcs, fbytes, BATCH, d_wall.ptr, Hc * Wc * 3, s))

                def gallery():
                    for f in range(BATCH):
                        ctx._check(lib.avx_gallery_compose_u8(ctx._h, descs[f], n_tiles, segp, len(seg), lay.strip_h, lay.pad, lay.cols, bg,
                                                              d_gal.ptr + f * Hg * Wg * 3, Hg, Wg, s))

                forms = {"gallery_x8": gallery, "wall": wall}
                try:
                    for run in forms.values():  # warm-up: code objects, workspaces, the clock ramp
                        for _ in range(3):
                            run()
                    got = ctx.download(d_wall, (BATCH, Hc, Wc, 3), np.uint8, stream=s)
                    want = ctx.download(d_gal, (BATCH, Hg, Wg, 3), np.uint8, stream=s)
                    if not np.array_equal(got[:, :Hg, :Wg], want):
                        raise SystemExit(f"wall_bench: the wall's canvases differ from the gallery's at {name}, {n_tiles} tiles, tile height {tile_height}")
                    times = {k: [] for k in forms}
                    for _ in range(args.reps):
                        for k, run in forms.items():
                            ctx.timer_start(s)
                            run()
                            times[k].append(ctx.timer_stop(s) * 1e3 / BATCH)  # ms per batch -> us per frame
                    moved = n_tiles * fbytes + Hc * Wc * 3  # bytes one sheet must move: every source read once, the canvas written once
                    med = {}
                    for k, us in times.items():
                        us = sorted(us)
                        med[k] = statistics.median(us)
                        emit({"bench": "kernels", "size": name, "tiles": n_tiles, "tile_height": tile_height, "form": k, "batch": BATCH, "reps": len(us),
                              "mode": mode.value, "staged": staged.value, "piece_px": piece.value, "lds_bytes": lds.value,
                              "us_per_frame_median": round(med[k], 1), "us_per_frame_min": round(us[0], 1), "us_per_frame_max": round(us[-1], 1),
                              "bytes_per_frame": moved, "tb_per_s_median": round(moved / med[k] / 1e6, 3)})
                    emit({"bench": "kernels", "size": name, "tiles": n_tiles, "tile_height": tile_height,
                          "gallery_x8_over_wall": round(med["gallery_x8"] / med["wall"], 2)})
                finally:
                    ctx.sync(s)
                    ctx.stream_destroy(s)
                    lib.avx_wall_layout_destroy(ctx._h, handle.value)
                    d_wall.free()
                    d_gal.free()
            d_src.free()


def stream(args):
    from animal_vision_amd.gallery import species_class
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.video import stream_op
    from animal_vision_amd.wall import WallStreamOp
    from animal_vision_amd.yuv import rgb_to_i420

    ctx = _need_gpu()
    emit = _emitter(args.out)
    for name, H, W in SIZES:
        if args.only and name not in args.only:
            continue
        nframes = args.frames if H < 2000 else max(BATCH, args.frames // 2)
        pool = rgb_to_i420(_pool(8, H, W))
        frames = [pool[k % 8] for k in range(nframes)]
        forms, opened = {}, []
        for batch in (1, BATCH):
            op = WallStreamOp([(n, species_class(n)()) for n in WALL], H, W, depth=3, batch=batch)
            pipe = FramePipeline(op, H, W, depth=3, batch=batch, io_format="i420")
            opened.append((op, pipe))
            forms[f"wall_batch{batch}"] = lambda pipe=pipe: pipe.run(iter(enumerate(frames)), lambda i, o: None).frames
            singles = []
            for n in WALL:
                sop = stream_op(species_class(n)(), H, W, 3, batch)
                spipe = FramePipeline(sop, H, W, depth=3, batch=batch, io_format="i420")
                opened.append((sop, spipe))
                singles.append(spipe)

            def four(singles=singles):
                for spipe in singles:  # one after the other: the four `video` runs
                    n = spipe.run(iter(enumerate(frames)), lambda i, o: None).frames
                return n

            forms[f"four_streams_batch{batch}"] = four
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
                emit({"bench": "stream", "size": name, "form": k, "species": WALL, "frames": nframes, "reps": len(v), "fps_median": round(med[k], 1),
                      "fps_min": round(v[0], 1), "fps_max": round(v[-1], 1)})
            emit({"bench": "stream", "size": name, **{f"wall_over_four_streams_batch{b}": round(med[f"wall_batch{b}"] / med[f"four_streams_batch{b}"], 2)
                                                      for b in (1, BATCH)}})
        finally:
            for op, pipe in opened:
                pipe.close()
                if hasattr(op, "close"):
                    op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["kernels", "stream"])
    ap.add_argument("--reps", type=int, default=None, help="repetitions per form (default 9 for kernels, 5 for stream)")
    ap.add_argument("--frames", type=int, default=48, help="stream: frames per timed run (halved at 4K)")
    ap.add_argument("--only", nargs="*", default=None, help="1080p and / or 4k")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 9 if args.cmd == "kernels" else 5
    if args.reps < 5:
        raise SystemExit("wall_bench: at least five repetitions per form")
    {"kernels": kernels, "stream": stream}[args.cmd](args)


if __name__ == "__main__":
    main()
