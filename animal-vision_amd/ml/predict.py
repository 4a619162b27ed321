"""Predictor harness around MSTPlusPlus: the semantics of the reference's
ml/MST_plus_plus/predict_code/predict_torch.py (predict_rgb_to_hsi_torch :249-310): float01 ->
reflect-pad H,W to a multiple of `stride` split on both sides (:171-183) -> NCHW -> model under fp16
-> crop -> HxWx31 float32.  Full-frame only: MI355X has 288 GB of HBM, and MST++'s spectral attention
contracts over every pixel of the frame, so the reference's OOM tile fallback (:199-235) is neither
needed nor equivalent."""
from __future__ import annotations

import weakref
from typing import Optional, Tuple

import numpy as np


def to_float01(img: np.ndarray) -> np.ndarray:
    """predict_torch.py:12-19."""
    if np.issubdtype(img.dtype, np.integer):
        return img.astype(np.float32) / 255.0
    x = img.astype(np.float32)
    if x.max() > 1.001:
        x = np.clip(x / 255.0, 0.0, 1.0)
    return x


def pad_amounts(H: int, W: int, mult: int) -> Tuple[int, int, int, int]:
    """(top, bottom, left, right) of predict_torch.py:22-34: total padding split floor/ceil."""
    if mult is None or mult <= 0:
        return 0, 0, 0, 0
    Hn, Wn = ((H + mult - 1) // mult) * mult, ((W + mult - 1) // mult) * mult
    py, px = Hn - H, Wn - W
    return py // 2, py - py // 2, px // 2, px - px // 2


def pad_to_multiple_reflect(x: np.ndarray, mult: int):
    pads = pad_amounts(x.shape[0], x.shape[1], mult)
    if pads == (0, 0, 0, 0):
        return x, pads
    t, b, l, r = pads
    return np.pad(x, ((t, b), (l, r), (0, 0)), mode="reflect"), pads


def crop_pads(x: np.ndarray, pads) -> np.ndarray:
    """predict_torch.py:37-40."""
    t, b, l, r = pads
    H, W = x.shape[:2]
    return x[t : H - b if b else H, l : W - r if r else W, :]


def reduced_size(H: int, W: int, hsi_scale, stride: int):
    """The size the network runs at for an H x W frame and HoneyBee(hsi_downsample=True, hsi_scale=s): (h, w) =
    (max(1, round(H s)), max(1, round(W s))), the rule of uv_helpers.py:169-170 (classic_rgb_to_hsi_scaled) and of
    planevm.spectral_planes.  None: the full-size route (hsi_scale None, or a frame the scale does not reduce).  ValueError when the
    scale is outside [0.05, 1) or the reduced frame is too small to be reflect-padded to a multiple of `stride` (a reflection cannot
    reach further than the frame it mirrors: every pad_amounts() entry must stay below the frame's extent)."""
    if hsi_scale is None:
        return None
    s = float(hsi_scale)
    if not 0.05 <= s < 1.0:
        raise ValueError(f"hsi_scale must be at least 0.05 and below 1 (got {hsi_scale!r})")
    h, w = max(1, int(round(H * s))), max(1, int(round(W * s)))
    if (h, w) == (H, W):
        return None
    t, b, l, r = pad_amounts(h, w, stride)
    if max(t, b) >= h or max(l, r) >= w:
        raise ValueError(f"hsi_scale={s:g} reduces the {H}x{W} frame to {h}x{w}, which cannot be reflect-padded to a multiple of {stride}: "
                         f"use a larger hsi_scale or a larger frame")
    return h, w


def check_bands(op) -> None:
    """The cube MST++ hands over has the model's 31 bands (400-700 nm, padded to a 32-wide group): a HoneybeeOp built for another band
    grid (HoneyBee(hsi_band_centers_nm=...)) would weight the wrong bands once padded to 32."""
    from .mst_plus_plus import DIM

    bands = op.weights.shape[1]
    if bands != DIM:
        raise ValueError(f"MST++ -> honeybee hand-off: the operator integrates {bands} bands, the network's cube has {DIM}")


class MSTPlusPlusPredictor:
    """RGB frame -> 31-band cube on the GPU.  weights: None (seeded random init: no checkpoint ships with the
    reference and there is no network), a path to a local .pth, or a state_dict."""

    def __init__(self, weights=None, *, seed: int = 0, half: bool = True, stride: int = 16, device: Optional[str] = None):
        import torch

        from .mst_plus_plus import MSTPlusPlus

        self.torch = torch
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.half = bool(half) and self.device.type == "cuda"
        self.stride = stride
        model = MSTPlusPlus()
        if weights is None:
            model.init_seeded(seed)
        elif isinstance(weights, (str, bytes)):
            model.load_reference_state_dict(torch.load(weights, map_location="cpu", weights_only=True), strict=False)
        else:
            model.load_reference_state_dict(weights)
        self._padded_ops = weakref.WeakKeyDictionary()  # HoneybeeOp -> its clone padded to 32 bands; by identity, dropped with the op (an id() key outlives it)
        self._catch_ops = weakref.WeakKeyDictionary()   # padded clone -> its tail fed catch planes as a 3-band cube (HoneybeeOp.catch_clone)
        self.model = model.to(self.device).eval()
        if self.half:
            self.model = self.model.half()
        self._prepared = False

    def prepare(self) -> "MSTPlusPlusPredictor":
        """Build every derived weight tensor of the model (packed MFMA fragments, stacked QKV, folded up-fuse weights, gather
        indices: MSTPlusPlus._prep fills its cache lazily with torch kernels on whichever stream runs the first frame) NOW, on
        the current stream, and wait for them: afterwards frames may be enqueued on any number of streams without one of them
        reading a cache entry another stream is still writing.  The derived tensors do not depend on the frame size, so one
        small frame through the same route builds them all.  Idempotent; a no-op on the CPU."""
        if self._prepared or self.device.type != "cuda":
            return self
        torch = self.torch
        with torch.cuda.device(self.device):
            probe = torch.zeros((32, 32, 3), dtype=torch.uint8, device=self.device)
            self.predict_device_nhwc(probe)
            torch.cuda.synchronize(self.device)
        self._prepared = True
        return self

    def predict_device_nhwc(self, frame_dev):
        """uint8 (H,W,3) torch tensor on the device -> (H, W, 32) contiguous channels-last cube: bands 0..30 and one
        zero padding channel (64-byte pixels; fp16 when half).  This is what the libavx hand-off consumes."""
        torch = self.torch
        H, W, _ = frame_dev.shape
        t, b, l, r = pad_amounts(H, W, self.stride)
        if self.half and frame_dev.dtype == torch.uint8 and self.stride % 8 == 0 and max(t, b) < H and max(l, r) < W and H > 1 and W > 1 and self.model.can_fuse_conv_in():
            y = self.model.forward_from_u8(frame_dev, (t, b, l, r))  # / 255, float16, reflect pad and conv_in in ONE kernel
            return y[0, t : t + H, l : l + W, :].contiguous()
        x = frame_dev.to(torch.float32).div_(255.0).permute(2, 0, 1).unsqueeze(0)  # 1x3xHxW
        if t or b or l or r:
            x = torch.nn.functional.pad(x, [l, r, t, b], mode="reflect")
        y = self.model.forward_nhwc(x.half() if self.half else x)
        return y[0, t : t + H, l : l + W, :].contiguous()

    def honeybee_device(self, frame_dev, op32, d_out, stream_handle, hsi_scale=None, work=None):
        """uint8 (H, W, 3) device frame -> honeybee frame in d_out (a DeviceBuffer of H*W*3 bytes), everything enqueued on torch's current stream
        (= stream_handle).  Where the fused kernels apply and op32.takes_catches(), the 31-band cube is never written: conv_out's epilogue integrates it
        into the three catch planes (+ their statistics) that the honeybee tail starts from; else the cube is handed over by data_ptr.  op32: the HoneybeeOp padded to
        32 bands (op.padded_clone(32)).  Returns the tensors that must stay alive until the stream has run (the caller records / keeps them).
        hsi_scale: the network runs on the frame reduced to reduced_size(H, W, hsi_scale, stride) and the catches are enlarged (_honeybee_reduced; `work`: its
        buffers, reduced_work(), lent by a caller that keeps them for this stream: those are not among the returned tensors); None, or a scale that does not reduce the frame, is the full-size route, launch for launch."""
        torch = self.torch
        H, W, _ = frame_dev.shape
        small = reduced_size(H, W, hsi_scale, self.stride)
        if small is not None:
            return self._honeybee_reduced(frame_dev, op32, d_out, stream_handle, small, work)
        t, b, l, r = pad_amounts(H, W, self.stride)
        fuse = (self.half and frame_dev.dtype == torch.uint8 and self.stride % 8 == 0 and max(t, b) < H and max(l, r) < W and H > 1 and W > 1
                and self.model.can_fuse_spectral() and op32.weights.shape == (3, 32) and op32.takes_catches())
        if fuse:
            planes, partials, n = self.model.forward_from_u8(frame_dev, (t, b, l, r), spectral=op32.weights)
            op32.run_device(None, d_out, 1, H, W, catches=(planes.data_ptr(), partials.data_ptr(), n), stream=stream_handle)
            return planes, partials
        cube = self.predict_device_nhwc(frame_dev)
        op32.run_device(None, d_out, 1, H, W, hsi_ptr=cube.data_ptr(), hsi_layout=0, hsi_dtype=1 if cube.dtype == torch.float16 else 0, stream=stream_handle)
        return (cube,)

    def reduced_work(self, H: int, W: int, small):
        """The buffers one reduced-resolution frame needs beside the network's own: the reduced frame, the enlarged catch planes and their
        statistics records (8 per CU, avx_honeybee_u8 source 2's limit).  A stream op allocates them once per slot."""
        torch = self.torch
        ncu = torch.cuda.get_device_properties(self.device).multi_processor_count
        return {"small": torch.empty((small[0], small[1], 3), dtype=torch.uint8, device=self.device),
                "planes": torch.empty((3, H, W), dtype=torch.float32, device=self.device),
                "partials": torch.empty((ncu * 8, 3, 2), dtype=torch.float64, device=self.device)}  # 16-byte records {float min, max; double sum}

    def _honeybee_reduced(self, frame_dev, op32, d_out, stream_handle, small, work=None):
        """HoneyBee(hsi_model=, hsi_downsample=True): classic_rgb_to_hsi_scaled (uv_helpers.py:155-183: INTER_AREA down -> converter -> INTER_LINEAR
        up) with the network as the converter.  The three catches are linear in the cube, so they are taken at the reduced size and the three planes
        are enlarged instead of 31 bands (as HoneyBee._visualize_staged does for the analytic converter):
          frame --avx_resize_hwc (uint8, INTER_AREA)--> h x w frame --MST++ + spectral integration--> 3 x h*w catches
                --avx_catch_planes_up--> 3 x H*W catches + their statistics --> the honeybee tail (source 2; else source 1 on the planes as a
                3-band planar cube with identity weights).
        The reduced frame is rounded to uint8 (the reference resizes the float image unrounded: at most half a code at the network's input), which is
        the frame `video --scale` hands the network and what the fused conv_in front end takes.  One stream, no host synchronisation."""
        import ctypes

        from .._lib import lib

        torch = self.torch
        if frame_dev.dtype != torch.uint8:
            raise NotImplementedError(f"the reduced-resolution MST++ route takes uint8 frames (got {frame_dev.dtype})")
        H, W, _ = frame_dev.shape
        h, w = small
        ctx = op32._ctx()
        own = work is None
        work = self.reduced_work(H, W, small) if own else work
        small_dev, planes, partials = work["small"], work["planes"], work["partials"]
        assert small_dev.shape == (h, w, 3) and planes.shape == (3, H, W) and op32.weights.shape == (3, 32)
        ctx._check(lib.avx_resize_hwc(ctx._h, frame_dev.data_ptr(), 2, H, W, 3, small_dev.data_ptr(), h, w, 3, stream_handle))
        pads = pad_amounts(h, w, self.stride)  # reduced_size() has checked that the reflection fits
        if self.half and self.stride % 8 == 0 and h > 1 and w > 1 and self.model.can_fuse_spectral():
            catches, _, _ = self.model.forward_from_u8(small_dev, pads, spectral=op32.weights)  # the reduced frame's own statistics are not used
            keep = (catches,)
        else:
            cube = self.predict_device_nhwc(small_dev)
            catches = torch.empty((3, h, w), dtype=torch.float32, device=cube.device)
            ctx._check(lib.avx_spectral_integrate(ctx._h, cube.data_ptr(), 0, 1 if cube.dtype == torch.float16 else 0, h, w, cube.shape[-1],
                                                  op32.weights.ctypes.data, 3, catches.data_ptr(), None, stream_handle))
            keep = (cube, catches)
        n = ctypes.c_int(0)
        ctx._check(lib.avx_catch_planes_up(ctx._h, catches.data_ptr(), h, w, planes.data_ptr(), H, W, partials.data_ptr(), ctypes.byref(n), stream_handle))
        if op32.takes_catches():
            op32.run_device(None, d_out, 1, H, W, catches=(planes.data_ptr(), partials.data_ptr(), n.value), stream=stream_handle)
        else:  # falsecolor_uv_mixed, blurs wider than 3 taps: the plane schedule forms its own statistics
            tail = self._catch_ops.get(op32)
            if tail is None:
                tail = self._catch_ops.setdefault(op32, op32.catch_clone())
            tail.run_device(None, d_out, 1, H, W, hsi_ptr=planes.data_ptr(), hsi_layout=1, hsi_dtype=0, stream=stream_handle)
        # buffers the caller lent live as long as its slot and are used on this stream alone: they are not handed back for record_stream (a tensor
        # recorded on a slot's stream and freed after that stream is destroyed makes the allocator record an event on a dead stream)
        return keep + (small_dev, planes, partials) if own else keep

    def predict_device(self, frame_dev):
        """uint8 (H,W,3) torch tensor on the device -> (31, H, W) contiguous tensor (fp16 when half)."""
        return self.predict_device_nhwc(frame_dev)[..., :31].permute(2, 0, 1).contiguous()

    def predict(self, image: np.ndarray) -> np.ndarray:
        """predict_rgb_to_hsi_torch for one image: HxWx3 (uint8 or float) -> HxWx31 float32."""
        torch = self.torch
        if self.device.type == "cuda" and image.dtype == np.uint8:  # the device route (what the honeybee hand-off runs): same kernels, same cube
            frame = torch.from_numpy(np.ascontiguousarray(image)).to(self.device)
            return self.predict_device_nhwc(frame)[..., :31].float().cpu().numpy()
        x01, pads = pad_to_multiple_reflect(to_float01(image), self.stride)
        xt = torch.from_numpy(np.ascontiguousarray(x01.transpose(2, 0, 1))[None]).to(self.device)
        y = self.model(xt.half() if self.half else xt.float())
        hsi = y[0].permute(1, 2, 0).float().cpu().numpy()
        return crop_pads(hsi, pads).astype(np.float32, copy=False)

    def honeybee(self, image: np.ndarray, op, hsi_scale=None) -> np.ndarray:
        """uint8 frame -> MST++ cube -> HoneybeeOp (csrc/uv.hip), the cube handed over on the device:
        the (H,W,32) channels-last tensor's data_ptr goes straight into avx_honeybee_u8 on torch's current stream.
        hsi_scale: the reduced-resolution route (honeybee_device)."""
        check_bands(op)
        torch = self.torch
        if self.device.type != "cuda":
            raise RuntimeError("MST++ -> libavx hand-off needs the GPU (no CPU path)")
        from ..runtime import DeviceBuffer

        H, W, _ = image.shape
        reduced_size(H, W, hsi_scale, self.stride)  # a reduced frame too small to pad: refused before anything is enqueued
        frame = torch.from_numpy(np.ascontiguousarray(image)).to(self.device)
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
        ctx = op._ctx()
        stream = torch.cuda.current_stream().cuda_stream
        op32 = self._padded_ops.get(op)
        if op32 is None:
            op32 = self._padded_ops.setdefault(op, op.padded_clone(32))  # the cube is channels-last, 31 bands in a 32-wide group
        keep = self.honeybee_device(frame, op32, DeviceBuffer(ctx, out.data_ptr(), out.numel(), owned=False), stream, hsi_scale=hsi_scale)
        res = out.cpu().numpy()  # synchronises: `keep` may go
        del keep
        return res


class MstHoneybeeStreamOp:
    """The north-star route (uint8 frame -> MST++ cube -> honeybee tail -> uint8 frame) as a frame-loop operator
    (pipeline.FramePipeline's protocol: slot_buffers(k) lends a slot's device frames, run_device(...) enqueues one frame on
    the slot's HIP stream).  torch's kernels and libavx's ride the SAME stream: the slot's stream is made torch's current
    stream for the duration of the call, and the cube goes from the network to csrc/uv.hip by data_ptr (no copy, no sync).
    hsi_scale: the reduced-resolution route (MSTPlusPlusPredictor.honeybee_device), with the reduced frame, the enlarged catch planes
    and their statistics records held per slot.  batch: frames per slot; the network runs them one after the other on the slot's stream."""

    def __init__(self, predictor: "MSTPlusPlusPredictor", bee_op, H: int, W: int, depth: int = 3, *, hsi_scale=None, batch: int = 1):
        check_bands(bee_op)
        torch = predictor.torch
        if predictor.device.type != "cuda":
            raise RuntimeError("MST++ -> libavx hand-off needs the GPU (no CPU path)")
        if batch < 1:
            raise ValueError(f"batch must be at least 1 (got {batch})")
        from ..runtime import DeviceBuffer

        self.pred, self.H, self.W = predictor, H, W
        self.hsi_scale, self.max_batch = hsi_scale, int(batch)
        small = reduced_size(H, W, hsi_scale, predictor.stride)  # ValueError before anything is launched
        self.ctx = bee_op._ctx()
        predictor.prepare()  # every derived weight exists and is complete before the slot streams start (they share the cache, unsynchronised)
        self._work = [predictor.reduced_work(H, W, small) if small is not None else None for _ in range(depth)]
        self._t_in = [torch.empty((self.max_batch, H, W, 3), dtype=torch.uint8, device=predictor.device) for _ in range(depth)]
        self._t_out = [torch.empty((self.max_batch, H, W, 3), dtype=torch.uint8, device=predictor.device) for _ in range(depth)]
        self._bufs = [(DeviceBuffer(self.ctx, a.data_ptr(), a.numel(), owned=False), DeviceBuffer(self.ctx, b.data_ptr(), b.numel(), owned=False))
                      for a, b in zip(self._t_in, self._t_out)]
        self._by_in = {bi.ptr: k for k, (bi, _) in enumerate(self._bufs)}
        self._bee = bee_op
        self._op32 = None
        self._streams = {}

    def slot_buffers(self, k: int):
        return self._bufs[k]

    def run_device(self, d_in, d_out, n_frames: int, H: int, W: int, stream=None):
        assert 1 <= n_frames <= self.max_batch and (H, W) == (self.H, self.W)
        torch = self.pred.torch
        k = self._by_in[d_in.ptr]
        ext = self._streams.get(stream)
        if ext is None:
            ext = self._streams.setdefault(stream, torch.cuda.ExternalStream(stream, device=self.pred.device))
        with torch.cuda.stream(ext):
            if self._op32 is None:
                self._op32 = self._bee.padded_clone(32)  # host-side tables only (uploaded per call through the workspace of `stream`)
            fbytes = H * W * 3
            for f in range(n_frames):
                for tns in self.pred.honeybee_device(self._t_in[k][f], self._op32, d_out.view(f * fbytes, fbytes), stream, hsi_scale=self.hsi_scale,
                                                     work=self._work[k]):
                    tns.record_stream(ext)

    def release_streams(self):
        """Called by pipeline.FramePipeline.close(): its slot streams are about to be destroyed, so the ExternalStream wrappers
        (and the allocator pools torch keyed by them) must not outlive them."""
        torch = self.pred.torch
        if self._streams:
            torch.cuda.synchronize(self.pred.device)
            self._streams.clear()
            torch.cuda.empty_cache()
