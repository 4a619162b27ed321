"""The digests of what the five colour difference entries of the deltae command write (csrc/delta_e.hip, receptor.hip, scielab.hip,
receptor_acuity.hip, itp.hip), for tests/test_deltae_family_digests_gpu.py: compute() runs a fixed set of small cases through the launch
functions of animal_vision_amd.metrics and returns {case id: sha256}.  A digest covers, in this order, for the launch ("heat", "map",
gain None, threshold 1.0) and then for ("plain", "side", 2.5, 0.0): the float32 value plane, the map and the raw bytes of the records as
downloaded (the float64 sum included: it is a function of H and W alone by design).  The frames are the seeded ones of the _*_ref.py
helpers, two frames a case (five for dE_ITP, whose generator fixes the count).  Run as a script, it prints the JSON."""
import hashlib
import json

import numpy as np

import _acuity_ref as A
import _deltae_ref as E
import _itp_ref as I
import _scielab_ref as S

LAUNCHES = (("heat", "map", None, 1.0), ("plain", "side", 2.5, 0.0))


def _digest(ctx, n, H, W, launch):
    """launch(d_map, d_rec, d_float, mode=, layout=, gain=, threshold=) enqueues one call on n frames of H x W."""
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES

    sha = hashlib.sha256()
    bufs = [ctx.malloc(n * H * W * 9), ctx.malloc(n * DELTA_E_RECORD_BYTES), ctx.malloc(n * H * W * 4)]
    try:
        d_map, d_rec, d_val = bufs
        for mode, layout, G, T in LAUNCHES:
            launch(d_map, d_rec, d_val, mode=mode, layout=layout, gain=G, threshold=T)
            sha.update(ctx.download(d_val, (n, H, W), np.float32).tobytes())
            sha.update(ctx.download(d_map, (n, H, W * (3 if layout == "side" else 1), 3), np.uint8).tobytes())
            sha.update(ctx.download(d_rec, (n * DELTA_E_RECORD_BYTES,), np.uint8).tobytes())
    finally:
        for d in bufs:
            d.free()
    return sha.hexdigest()


def _pair_digest(ctx, a, b, launch_fn, **kw):
    """A case of two uint8 stacks N x H x W x 3 through delta_e_launch, scielab_launch or receptor_delta_launch."""
    n, H, W = a.shape[:3]
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    try:
        return _digest(ctx, n, H, W, lambda d_map, d_rec, d_val, **opt: launch_fn(ctx, d_a, d_b, n, H, W, d_map, d_rec, d_float=d_val, **opt, **kw))
    finally:
        d_a.free(), d_b.free()


def _itp_digest(ctx, case):
    from animal_vision_amd.metrics import HdrFrames, ItpSide, itp_delta_launch

    H, W = case[:2]
    n = len(I.KINDS)
    sides, bufs = [], []
    try:
        for ref in I.case_sides(case)[:2]:
            if ref[0] == "sdr":
                bufs.append(ctx.upload(ref[1]))
                sides.append(ItpSide(bufs[-1]))
            else:
                _, payload, fmt, transfer, rng = ref
                h = HdrFrames(payload, fmt, H, W, transfer, rng)
                bufs.extend([ctx.upload(h.payload), ctx.malloc(n * H * W * 3)])
                h.decode().launch(ctx, bufs[-2], bufs[-1], n, H, W)  # the panel frames of the map
                sides.append(ItpSide(bufs[-2], fmt, transfer, rng, bufs[-1]))
        return _digest(ctx, n, H, W, lambda d_map, d_rec, d_val, **opt: itp_delta_launch(ctx, sides[0], sides[1], n, H, W, d_map, d_rec, d_float=d_val, **opt))
    finally:
        for d in bufs:
            d.free()


def _two(H, W):
    """Two frame pairs of _deltae_ref.frames: a near copy and unrelated noise."""
    named = {name: (a, b) for name, a, b in E.frames(H, W, 1000 * H + W)}
    return (np.stack([named[k][i] for k in ("near", "random")]) for i in (0, 1))


def compute():
    from animal_vision_amd.metrics import Observer, delta_e_launch, observer_for, receptor_delta_launch, scielab_launch
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    out = {}
    observers = (observer_for("Dog", (0.05, 0.05)), observer_for("HoneyBee", (0.13, 0.06, 0.12)))
    for H, W in ((29, 37), (72, 64)):  # the byte path in one chunk; the 16-byte path in two
        a, b = _two(H, W)
        out[f"de00-{H}x{W}"] = _pair_digest(ctx, a, b, delta_e_launch)
        for obs in observers:
            out[f"receptor-{obs.name}-{H}x{W}"] = _pair_digest(ctx, a, b, receptor_delta_launch, observer=obs)
    a, b = _two(29, 37)
    out["receptor-four-29x37"] = _pair_digest(ctx, a, b, receptor_delta_launch, observer=Observer("four", A.FOUR, (0.08,) * 4))
    for H, W, ppd in ((5, 7, 60.0), (70, 530, 22.5)):  # the radius exceeds the frame; several row and column tiles, W no multiple of 4
        noise, ramp = S.frame("noise", H, W, 1000 * H + W), S.frame("ramp", H, W, 0)
        a, b = np.stack([noise, ramp]), np.stack([S.jitter(noise, 1000 * H + W + 1), S.frame("primaries", H, W, 1000 * H + W + 2)])
        out[f"scielab-{H}x{W}-ppd{ppd:g}"] = _pair_digest(ctx, a, b, scielab_launch, ppd=ppd)
    for obs, H, W, sigma in ((observers[0], 5, 7, 3.5), (observers[0], 70, 530, 1.0), (observers[1], 70, 530, 3.5)):
        a, b = (x[[0, 2]] for x in A.frames(H, W))  # noise against noise, noise against its near copy
        out[f"acuity-{obs.name}-{H}x{W}-sigma{sigma:g}"] = _pair_digest(ctx, a, b, receptor_delta_launch, observer=obs, acuity=sigma)
    for case in I.CASES:
        out[f"itp-{I.case_id(case)}"] = _itp_digest(ctx, case)
    return out


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(compute(), indent=1))
