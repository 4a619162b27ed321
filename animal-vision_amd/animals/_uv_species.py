"""Common machinery of the UV species written against the plane-program backend vocabulary (planevm.py).

A species implements `render(be, image)` once; `visualize` records it for the frame size on a DeviceBackend the
first time it sees that size and replays the recorded device calls afterwards (species are stateless between
frames, SURVEY 8b: only constructor constants and O(bands)/O(H)/O(W) tables enter the recording)."""
from typing import Dict, Optional, Tuple

import numpy as np

from .animal import Animal


class UVSpecies(Animal):
    """Base class: same `visualize(image) -> (baseline, out)` contract as the reference's species."""

    _MAX_PLANS = 4
    BATCH_CAPACITY = 8  # frames a batched plan is recorded for unless the caller says otherwise (shorter batches replay it)

    def render(self, be, image: np.ndarray) -> None:  # pragma: no cover - abstract
        """Species with a frame-dependent branch take a third argument: the value `variant()` returned."""
        raise NotImplementedError

    def variant(self, image: np.ndarray, probes, **kw):
        """A hashable that selects between recorded plans when the reference branches on frame content
        (rat_uv.py:100-105); `probes` supplies the frame statistics (device: planevm.DeviceProbes)."""
        return None

    def _plan(self, image: np.ndarray, variant=None, frames: int = 1):
        """The recorded plan for this frame size / variant / batch capacity (`frames`: how many frames one replay takes)."""
        from ..planevm import DeviceBackend

        plans: Dict[tuple, object] = self.__dict__.setdefault("_plans", {})
        floats = image.dtype != np.uint8
        key = (image.shape[0], image.shape[1], variant, floats) if frames == 1 else (image.shape[0], image.shape[1], variant, floats, frames)
        be = plans.get(key)
        if be is None:
            if len(plans) >= self._MAX_PLANS:
                plans.pop(next(iter(plans))).close()
            be = DeviceBackend(image.shape[0], image.shape[1], float_frames=floats, frames=frames)
            if variant is None:
                self.render(be, image)
            else:
                self.render(be, image, variant)
            be.flush()
            plans[key] = be
        return be

    def visualize(self, image: np.ndarray, **kw) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        assert isinstance(image, np.ndarray), "Input must be a numpy ndarray."
        assert image.ndim == 3 and image.shape[2] == 3, "Input must be HxWx3 RGB."
        if image.dtype != np.uint8 and not np.issubdtype(image.dtype, np.floating):
            raise NotImplementedError(f"{type(self).__name__}: device path implemented for uint8 and float frames, got {image.dtype}")
        from ..planevm import DeviceProbes

        return self._plan(image, self.variant(image, DeviceProbes, **kw)).run(image)

    def visualize_batch(self, frames: np.ndarray, *, capacity: Optional[int] = None, **kw) -> Tuple[np.ndarray, np.ndarray]:
        """N uint8 frames (N x H x W x 3) -> (baselines, outs), both N x H x W x 3 and byte for byte what N `visualize` calls
        return, in one launch chain per batch instead of one per frame (planevm.DeviceBackend(frames=...)).

        The plan is recorded for `capacity` frames (default: BATCH_CAPACITY, whatever N is, so that one plan per size serves
        every batch length; at most 16) and cached next to the single-frame plans; longer inputs are split, shorter batches
        replay the same plan.  A species whose plan depends on the frame
        (RatUV mode="auto") is evaluated per frame, and the frames of each variant run as their own batch."""
        from .. import _lib
        from ..planevm import DeviceProbes

        assert isinstance(frames, np.ndarray), "Input must be a numpy ndarray."
        assert frames.ndim == 4 and frames.shape[3] == 3 and frames.shape[0] >= 1, "Input must be NxHxWx3 RGB."
        if frames.dtype != np.uint8:
            if np.issubdtype(frames.dtype, np.floating):
                raise NotImplementedError(f"{type(self).__name__}: batched device path implemented for uint8 frames, got {frames.dtype}")
            raise NotImplementedError(f"{type(self).__name__}: device path implemented for uint8 and float frames, got {frames.dtype}")
        n = frames.shape[0]
        cap = self.BATCH_CAPACITY if capacity is None else int(capacity)
        if not 1 <= cap <= _lib.AVX_EW_MAX_FRAMES:
            raise ValueError(f"capacity={capacity}: a batched plan holds 1..{_lib.AVX_EW_MAX_FRAMES} frames")
        groups: Dict[object, list] = {}
        for i in range(n):
            groups.setdefault(self.variant(frames[i], DeviceProbes, **kw), []).append(i)
        bases, outs = np.empty_like(frames), np.empty_like(frames)
        for variant, idx in groups.items():
            be = self._plan(frames[idx[0]], variant, frames=cap)
            for j in range(0, len(idx), cap):
                part = idx[j:j + cap]
                bases[part], outs[part] = be.run_batch(frames[part])
        return bases, outs


class SpeciesStreamOp:
    """Adapter that lets pipeline.FramePipeline / run_video stream uint8 frames through a UV species: one recorded
    plan per pipeline slot (each owns its device frames, which the pipeline copies into / out of directly), replayed
    on the slot's stream.  `output`: "out" (the stylised frame) or "baseline".  Species whose plan depends on frame
    content (RatUV's mode="auto") need the branch fixed by `variant`.  batch=N: every slot's plan holds N frames
    (DeviceBackend(frames=N)); the lent buffers are N contiguous frames and run_device takes 1 <= n_frames <= N."""

    def __init__(self, species: UVSpecies, H: int, W: int, *, depth: int = 3, variant=None, ctx=None, batch: int = 1):
        from ..planevm import DeviceBackend

        self.species, self.H, self.W, self.ctx = species, int(H), int(W), ctx
        self.batch = self.max_batch = int(batch)
        probe = np.zeros((H, W, 3), np.uint8)
        self.plans = []
        for _ in range(depth):
            be = DeviceBackend(H, W, ctx, frames=self.batch)
            if variant is None:
                species.render(be, probe)
            else:
                species.render(be, probe, variant)
            be.flush()
            self.plans.append(be)
        self.ctx = self.plans[0].ctx
        self._by_in = {be.d_in.ptr: be for be in self.plans}

    def slot_buffers(self, k: int):
        be = self.plans[k]
        return be.d_in, be.d_out

    def slot_baseline(self, k: int):
        """Slot k's baseline frame (uint8 HxWx3 on the device): what visualize() returns first, the panorama-warped input
        (FramePipeline(split_baseline=True) composes the split frame against it)."""
        return self.plans[k].d_base

    def run_device(self, d_in, d_out, n_frames: int, H: int, W: int, stream=None):
        assert 1 <= n_frames <= self.batch and (H, W) == (self.H, self.W)
        self._by_in[d_in.ptr].run_device(stream, n_frames)

    def close(self):
        for be in self.plans:
            be.close()
        self.plans = []


def default_lambdas(lambdas) -> np.ndarray:
    """The 300-700 nm / 81-band grid every UV species but HoneyBee defaults to (e.g. reindeer.py:56-58)."""
    lam = np.asarray(lambdas, dtype=np.float32) if lambdas is not None else np.linspace(300.0, 700.0, 81, dtype=np.float32)
    assert lam.ndim == 1 and lam.size >= 10, "lambdas must be a 1D vector of wavelengths (nm)."
    return lam


def snow_glare_tone_compress(be, x, *, strength: float, knee: float = 0.8):
    """uv_helpers.py:111-121 on one plane."""
    if strength <= 0.0:
        return x
    x = be.clip01(x)
    t = (x - knee) / (1.0 - knee)
    return be.where(x <= knee, x, knee + (1.0 - knee) * (t / (1.0 + strength * t)))


def radial_sigmoid(be, *, radius: float, softness: float):
    """The peripheral blend weight several species share (e.g. goldfish.py:165-170, mantis_shrimp.py:270-273)."""
    yy = be.row(np.linspace(-1.0, 1.0, be.H, dtype=np.float32))
    xx = be.col(np.linspace(-1.0, 1.0, be.W, dtype=np.float32))
    r = be.sqrt(xx * xx + yy * yy)
    return 1.0 / (1.0 + be.exp(-softness * (r - radius)))
