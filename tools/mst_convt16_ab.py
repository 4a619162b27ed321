"""The decoder upsampling kernels on K = 16 MFMAs against the K = 8 ones, and the whole-line K = 16 form (round 13) against both, kernel against kernel
(DESIGN §4.3).  Not part of bench.py.

  timeout -k 10 300 python tools/mst_convt16_ab.py --out ab.jsonl

One process, the 4K route's two decoder sizes (540 x 960 x 128 -> 1080 x 1920 x 64 and 1080 x 1920 x 64 -> 2160 x 3840 x 32), random inputs (the
arithmetic does not depend on them).  Per size the forms are launched alternately, `--launches` times each after a warm-up, every launch between
two stream events of its own with the queue kept full; the median, minimum and maximum per form go out as one JSON line.  A form is what the
route launches for the step: the fused transposed conv (+ the block's Gram pass, standalone or as the epilogue, and the partial reduction)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    ap.add_argument("--forms", default=None, help="comma-separated forms to launch (default: all): a counter pass or a trace of a few kernels without the others' launches in it")
    args = ap.parse_args()

    import torch

    from animal_vision_amd.ml.mst_plus_plus import _AVX, pack_fragments, pack_fragments16, pack_qkv16

    if not torch.cuda.is_available():
        raise SystemExit("mst_convt16_ab: needs a GPU")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    out = open(args.out, "w") if args.out else None
    for c, h, w in ((128, 540, 960), (64, 1080, 1920)):
        ch, heads = c // 2, c // 64
        x = torch.randn(1, h, w, c, device=dev).half()
        skip = torch.randn(1, 2 * h, 2 * w, ch, device=dev).half()
        taps = [(torch.randn(c, ch, device=dev) * 0.1).half() for _ in range(4)]
        wsk = (torch.randn(ch, ch, device=dev) * 0.1).half()
        bias = torch.randn(ch, device=dev) * 0.1
        wqk = pack_qkv16((torch.randn(ch, 3 * ch, device=dev) * 0.2).half())
        p8 = torch.stack([pack_fragments(t, True) for t in taps]).contiguous()
        p16 = torch.stack([pack_fragments16(t, halfrow=True) for t in taps]).contiguous()
        s8, s16 = pack_fragments(wsk, True), pack_fragments16(wsk, halfrow=True)

        def k8_gram():
            if c == 64:
                return _AVX.convt2x2_gram(x, p8, bias, skip, s8, wqk)[0]
            o = _AVX.convt2x2(x, p8, bias, skip, s8)
            _AVX.qkv_gram(o.reshape(1, 4 * h * w, ch), wqk, heads, want_v=False, k16=True)
            return o

        forms = {
            "k8_fuse": lambda: _AVX.convt2x2(x, p8, bias, skip, s8),
            "k16_fuse": lambda: _AVX.convt2x2_16(x, p16, bias, skip, s16),
            "k8_fuse+gram": k8_gram,
            "k16_fuse_gram": lambda: _AVX.convt2x2_16_gram(x, p16, bias, skip, s16, wqk)[0],
            "k16_fuse_ln": lambda: _AVX.convt2x2_16(x, p16, bias, skip, s16, lines=True),  # round 13: skip and output rows as whole 1 KB runs through LDS
            "k16_fuse_gram_ln": lambda: _AVX.convt2x2_16_gram(x, p16, bias, skip, s16, wqk, lines=True)[0],
        }
        if args.forms:
            want = args.forms.split(",")
            unknown = [k for k in want if k not in forms]
            if unknown:
                raise SystemExit(f"mst_convt16_ab: unknown form(s) {unknown}; known: {sorted(forms)}")
            forms = {k: f for k, f in forms.items() if k in want}
        for f in forms.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        ev = {k: [] for k in forms}
        for _ in range(args.launches):
            for k, f in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                ev[k].append((a, b))
        torch.cuda.synchronize()
        nbytes = 2 * (h * w * c + 2 * 4 * h * w * ch)  # x and skip read, out written
        for k, pairs in ev.items():
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)
            med = statistics.median(us)
            rec = {"C": c, "in_hw": [h, w], "form": k, "launches": len(us), "us_median": round(med, 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1),
                   "conv_bytes": nbytes, "TBps_median": round(nbytes / med / 1e6, 2)}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
