"""Time of the colour difference kernels.  Not part of bench.py.

  python tools/deltae_bench.py kernel [--reps 7] [--ppd 60 [--ppd 30 ...]] [--observer Dog [--observer HoneyBee ...]]
                                      [--acuity species [--acuity 1.0 ...]] [--edges [--smooth R:KEEP:ITER ...]] [--itp]
      avx_delta_e_u8 on frames resident on the device, 4K and 1080p, batches of 8: records only (no map), the heat map, the heat map
      side by side, and records only on a pair whose upper half is identical (those pixels are 0 by definition and skip the
      arithmetic), interleaved in one process with avx_frame_metrics_u8(with_ssim = 1) on the same frames -- per repetition each form
      once, each between its own pair of stream events (the record memset and the final launch included), after one warm-up call of
      each.  One JSON line per (size, form): median (min-max) in us per frame, ns per pixel, and the ratio to the SSIM record kernel.
      The frames are noise against the same noise +-2 codes: fewer than 1 % of the pixels are equal, so every wave does the arithmetic.
      Each --ppd X adds avx_scielab_u8 at X pixels per degree to the same interleaved repetitions, records only and with the heat map
      (the row pass, the column pass and the final launch between one pair of events); its lines also carry the ratio to the plain dE
      records and the fused multiply-adds per pixel pair of the two filter passes, 28 (2 ceil(X / 2) + 1).
      Each --observer NAME adds avx_receptor_delta_u8 for that observer (Weber fractions 0.05 each, 0.13,0.06,0.12 for HoneyBee: they
      are kernel arguments and do not change the work) to the same interleaved repetitions: records only, with the heat map, and side
      by side; its lines also carry the ratio to the plain dE form of the same outputs.
      Each --acuity SIGMA|species adds avx_receptor_acuity_u8 at that sigma for every --observer (`species`: the observer's own,
      skipped with a note for an observer without a Gaussian acuity) to the same interleaved repetitions, records only and with the
      heat map; its lines also carry the ratio to the observer's per-pixel records, the taps, and the fused multiply-adds per pixel pair
      of the two blur passes by arithmetic -- 6 planes x k taps x (1 + (32 + 2R) / 32): the column pass, and the row pass on the tile's
      32 rows and its 2R halo rows -- with the rate they imply.
      --edges adds avx_receptor_edges_u8 on the A frames for every --observer to the same interleaved repetitions,
      records only: at every --acuity sigma that the observer takes and without blur, at steps 1 and 8, chromatic and either (the
      luminance channel is the observer's last class at e_L = 0.1; it is a kernel argument and does not change the work); its lines
      also carry the ratio to avx_receptor_acuity_u8's records at the same sigma (which blurs six planes, this one three) or, without
      blur, to avx_receptor_delta_u8's, and the blurred pixels per owned pixel by arithmetic, 2048 / ((64 - 2D) (32 - 2D)).
      Each --smooth R:KEEP:ITER (with --edges) adds avx_receptor_edges_smooth_u8 beside every step-1 edges form, on
      the same frames in the same repetitions, and once per such form the same entry with ITER = 0 (the planes route without a
      smoothing launch: the front and the back kernel); its lines also carry the ratio to the fused edges form, and the time of one
      smoothing launch as (this form - the ITER = 0 form) / ITER.  The frames are noise: no window holds m exact zeros, so every pixel
      runs the whole selection.
      --itp adds avx_itp_delta to the same interleaved repetitions, records only: p010le PQ against p010le PQ, p010le
      HLG against p010le HLG (noise payloads against the same samples +-2 codes, so every wave does the arithmetic) and the PQ payload
      against the 8-bit frames as an SDR side at 203 nits, and the PQ pair once more with the heat map; its lines also carry the
      ratio to the plain dE records, the bytes of the two sides per pixel and the time those bytes take at the 6.29 TB/s copy rate.
  python tools/deltae_bench.py command [--frames 32] [--reps 3] [--dir DIR] [--ppd X]
      Two 4K nv12 files of `frames` frames in DIR (default: /dev/shm when there is one, so they are read from and written to memory)
      through python -m animal_vision_amd.deltae's main(), --batch 8 --depth 2: no OUT (statistics only), heat into a raw nv12 file (the
      map encoded on the device, 1.5 B/px back across PCIe), heat side by side into nv12, and heat into a .npy file (RGB, 3 B/px
      back): frames per second of the whole command (read, upload, decode, dE, encode, download, write), `reps` runs each after one
      warm-up run.  With --ppd X the statistics-only and the nv12 heat runs are repeated with --ppd X."""
import argparse
import contextlib
import io
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}


def _pair(n, H, W, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-2, 3, a.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    return a, b


def _smooth(text):
    r, keep, it = text.split(":")
    return int(r), float(keep), int(it)


def kernel(args):
    from animal_vision_amd.dichromat import cv_auto_ksize
    from animal_vision_amd.metrics import (DELTA_E_RECORD_BYTES, RECORD_BYTES, ItpSide, check_acuity, delta_e_launch, frame_metrics_launch, itp_delta_launch,
                                           observer_for, receptor_delta_launch, receptor_edges_launch, scielab_launch, species_acuity)
    from animal_vision_amd.runtime import get_context

    ctx, n = get_context(), 8
    for name, (H, W) in (("4k", SIZES["4k"]), ("1080p", SIZES["1080p"])):
        a, b = _pair(n, H, W)
        half = b.copy()
        half[:, : H // 2] = a[:, : H // 2]
        d_a, d_b, d_half, d_out = ctx.upload(a), ctx.upload(b), ctx.upload(half), ctx.malloc(3 * n * H * W * 3)
        d_rec, d_metrics = ctx.malloc(n * DELTA_E_RECORD_BYTES), ctx.malloc(n * RECORD_BYTES)

        def route(d_other, d_map, layout):
            return lambda: delta_e_launch(ctx, d_a, d_other, n, H, W, d_map, d_rec, mode="heat", layout=layout)

        def filtered(ppd, d_map):
            return lambda: scielab_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, ppd=ppd, mode="heat", layout="map")

        def receptor(obs, d_map, layout):
            return lambda: receptor_delta_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, observer=obs, mode="heat", layout=layout)

        def blurred(obs, sigma, d_map):
            return lambda: receptor_delta_launch(ctx, d_a, d_b, n, H, W, d_map, d_rec, observer=obs, mode="heat", layout="map", acuity=sigma)

        def edges(obs, sigma, step, channel, smooth=None):
            return lambda: receptor_edges_launch(ctx, d_a, n, H, W, None, d_rec, observer=obs, achromatic=((obs.n_receptors,), 0.1), channel=channel,
                                                 acuity=sigma or None, step=step, smooth=smooth)

        forms = [("records", route(d_b, None, "map")), ("heat map", route(d_b, d_out, "map")), ("heat side", route(d_b, d_out, "side")),
                 ("records, upper half identical", route(d_half, None, "map"))]
        for ppd in args.ppd or []:
            forms += [(f"scielab records, ppd {ppd:g}", filtered(ppd, None)), (f"scielab heat map, ppd {ppd:g}", filtered(ppd, d_out))]
        for who in args.observer or []:
            obs = observer_for(who, (0.13, 0.06, 0.12) if who == "HoneyBee" else (0.05, 0.05))
            forms += [(f"receptor {who} {what}", receptor(obs, d_map, layout))
                      for what, d_map, layout in (("records", None, "map"), ("heat map", d_out, "map"), ("heat side", d_out, "side"))]
            sigmas = [0.0]
            for text in args.acuity or []:
                try:
                    sigma = species_acuity(who) if text == "species" else check_acuity(float(text))
                except ValueError as e:
                    print(f"deltae_bench: --acuity {text} skipped for {who}: {e}", file=sys.stderr)
                    continue
                sigmas.append(sigma)
                forms += [(f"acuity {who} sigma {sigma:g} records", blurred(obs, sigma, None)), (f"acuity {who} sigma {sigma:g} heat map", blurred(obs, sigma, d_out))]
            if args.edges:
                forms += [(f"edges {who} sigma {sigma:g} step {step} {channel} records", edges(obs, sigma, step, channel))
                          for sigma in sigmas for step in (1, 8) for channel in ("chromatic", "either")]
                for sigma in sigmas if args.smooth else []:
                    for channel in ("chromatic", "either"):
                        forms.append((f"smooth {who} sigma {sigma:g} step 1 {channel} 1:1:0 records", edges(obs, sigma, 1, channel, (1, 1.0, 0))))
                        forms += [(f"smooth {who} sigma {sigma:g} step 1 {channel} {sm[0]}:{sm[1]:g}:{sm[2]} records", edges(obs, sigma, 1, channel, sm))
                                  for sm in args.smooth]
        extra = []
        if args.itp:
            rng = np.random.default_rng(1)
            ya = rng.integers(0, 1024, (n, H * W * 3 // 2), dtype=np.int16)  # p010le: 1.5 samples per pixel, the value in the top 10 bits
            yb = np.clip(ya + rng.integers(-2, 3, ya.shape, dtype=np.int16), 0, 1023)
            d_ya, d_yb, d_pan = ctx.upload((ya << 6).astype("<u2")), ctx.upload((yb << 6).astype("<u2")), ctx.upload(a)
            extra = [d_ya, d_yb, d_pan]

            def itp(sa, sb, d_map):
                return lambda: itp_delta_launch(ctx, sa, sb, n, H, W, d_map, d_rec, mode="heat", layout="map")

            for tr in ("pq", "hlg"):
                forms.append((f"itp {tr} - {tr} records", itp(ItpSide(d_ya, "p010le", tr), ItpSide(d_yb, "p010le", tr), None)))
            forms += [("itp pq - sdr records", itp(ItpSide(d_ya, "p010le", "pq"), ItpSide(d_b), None)),
                      ("itp pq - pq heat map", itp(ItpSide(d_ya, "p010le", "pq", d_panel=d_pan), ItpSide(d_yb, "p010le", "pq", d_panel=d_pan), d_out))]
        forms.append(("ssim record", lambda: frame_metrics_launch(ctx, d_a, d_b, n, H, W, d_metrics, ssim=True)))
        times = [[] for _ in forms]
        for _, r in forms:  # warm-up: code objects are loaded and the workspaces are sized here
            r()
        ctx.sync()
        for _ in range(args.reps):
            for k, (_, r) in enumerate(forms):
                ctx.timer_start()
                r()
                times[k].append(ctx.timer_stop() * 1e3 / n)
        record, plain = float(np.median(times[-1])), float(np.median(times[0]))
        for (form, _), t in zip(forms, times):
            med = float(np.median(t))
            line = {"size": name, "form": form, "batch": n, "reps": args.reps, "us_per_frame_median": round(med, 1), "us_per_frame_min": round(min(t), 1),
                    "us_per_frame_max": round(max(t), 1), "ns_per_px": round(med * 1e3 / (H * W), 4), "over_ssim_record_kernel": round(med / record, 2)}
            if form.startswith("scielab"):
                fma = 28 * (2 * math.ceil(float(form.rsplit(" ", 1)[1]) / 2) + 1)  # 7 terms x 2 sides x 2 passes, per tap
                line.update(over_plain_records=round(med / plain, 2), filter_fma_per_px=fma, filter_tflops=round(2 * fma * H * W / med * 1e-6, 2))
            if form.startswith("receptor"):
                same = {"records": 0, "map": 1, "side": 2}[form.rsplit(" ", 1)[1]]  # the plain dE form with the same outputs
                line.update(over_plain_same_outputs=round(med / float(np.median(times[same])), 2))
            if form.startswith("acuity"):
                who, sigma = form.split(" ")[1], float(form.split(" ")[3])
                k = cv_auto_ksize(sigma)
                fma = 6 * k * (1 + (32 + (k - 1)) / 32)
                base = [t2 for (f2, _), t2 in zip(forms, times) if f2 == f"receptor {who} records"][0]
                line.update(over_receptor_records=round(med / float(np.median(base)), 2), taps=k, blur_fma_per_px=round(fma, 1),
                            blur_tflops=round(2 * fma * H * W / med * 1e-6, 2))
            if form.startswith("edges"):
                who, sigma, step = form.split(" ")[1], float(form.split(" ")[3]), int(form.split(" ")[5])
                pair = f"acuity {who} sigma {sigma:g} records" if sigma else f"receptor {who} records"
                base = [t2 for (f2, _), t2 in zip(forms, times) if f2 == pair][0]
                line.update(pair_form=pair, over_pair_records=round(med / float(np.median(base)), 2),
                            blurred_px_per_owned_px=round(2048 / ((64 - 2 * step) * (32 - 2 * step)), 2))
            if form.startswith("smooth"):
                head, setting = form.rsplit(" ", 2)[0], form.split(" ")[-2]
                fused = [t2 for (f2, _), t2 in zip(forms, times) if f2 == "edges" + head[len("smooth"):] + " records"][0]
                line.update(over_fused_edges=round(med / float(np.median(fused)), 2))
                iterations = int(setting.rsplit(":", 1)[1])
                if iterations:
                    bare = [t2 for (f2, _), t2 in zip(forms, times) if f2 == f"{head} 1:1:0 records"][0]
                    line.update(front_and_back_us_per_frame=round(float(np.median(bare)), 1),
                                smooth_us_per_frame_and_iteration=round((med - float(np.median(bare))) / iterations, 1))
            if form.startswith("itp"):
                nbytes = 6.0  # 3 B/px of p010le on either side, or 3 B/px of p010le and 3 B/px of RGB
                line.update(over_plain_records=round(med / plain, 2), side_bytes_per_px=nbytes, us_per_frame_at_6p29_TBps=round(nbytes * H * W / 6.29e6, 1))
            print(json.dumps(line), flush=True)
        for d in [d_a, d_b, d_half, d_out, d_rec, d_metrics] + extra:
            d.free()


def command(args):
    from animal_vision_amd import deltae
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
        argv = [os.path.join(d, "a.yuv"), os.path.join(d, "b.yuv")]
        opts = ["--pix-fmt", "nv12", "--size", f"{W}x{H}", "--batch", "8", "--csv", os.path.join(d, "de.csv")]
        runs = [(None, []), ("out.yuv", ["--depth", "2"]), ("out.yuv", ["--depth", "2", "--layout", "side"]), ("out.npy", ["--depth", "2"])]
        if args.ppd is not None:
            runs += [(None, ["--ppd", f"{args.ppd:g}"]), ("out.yuv", ["--depth", "2", "--ppd", f"{args.ppd:g}"])]
        for out, extra in runs:
            fps = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                with contextlib.redirect_stderr(io.StringIO()):
                    status = deltae.main(argv + ([os.path.join(d, out)] if out else []) + opts + extra)
                dt = time.perf_counter() - t0
                assert status == 0, status
                if out:
                    os.remove(os.path.join(d, out))
                if rep:  # the first run is the warm-up
                    fps.append(args.frames / dt)
            print(json.dumps({"command": "deltae", "size": "4k", "pix_fmt": "nv12", "frames": args.frames, "batch": 8, "depth": 2,
                              "sink": "none" if out is None else ("nv12" if out.endswith(".yuv") else "npy"), "options": extra, "reps": args.reps,
                              "fps_median": round(float(np.median(fps)), 1), "fps_min": round(min(fps), 1), "fps_max": round(max(fps), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--reps", type=int, default=7)
    k.add_argument("--ppd", type=float, action="append", default=None, help="add avx_scielab_u8 at this many pixels per degree (repeatable)")
    k.add_argument("--observer", action="append", default=None, metavar="NAME",
                   help="add avx_receptor_delta_u8 for this observer, a dichromat's display name or HoneyBee (repeatable)")
    k.add_argument("--acuity", action="append", default=None, metavar="SIGMA|species",
                   help="add avx_receptor_acuity_u8 at this sigma in pixels, or at each observer's own, for every --observer (repeatable)")
    k.add_argument("--edges", action="store_true",
                   help="add avx_receptor_edges_u8 for every --observer: at every --acuity sigma and without blur, steps 1 and 8, chromatic and either")
    k.add_argument("--smooth", action="append", default=None, metavar="R:KEEP:ITER", type=_smooth,
                   help="with --edges: add avx_receptor_edges_smooth_u8 at this setting beside every step-1 edges form (repeatable)")
    k.add_argument("--itp", action="store_true", help="add avx_itp_delta: p010le PQ and HLG pairs, and PQ against an SDR side")
    c = sub.add_parser("command")
    c.add_argument("--frames", type=int, default=32)
    c.add_argument("--reps", type=int, default=3)
    c.add_argument("--dir", default=None)
    c.add_argument("--ppd", type=float, default=None, help="repeat the statistics-only and the nv12 heat runs with --ppd")
    args = ap.parse_args()
    {"kernel": kernel, "command": command}[args.cmd](args)


if __name__ == "__main__":
    main()
