"""The dichromat species (reference: animals/{dog,cat,...,tiger}.py), all on the fused HIP kernel.

Each class keeps the reference's surface: no-argument constructor, `visualize(image) ->
(baseline, out)` with `baseline is image` (dog.py:61) and out.dtype == image.dtype.
Parameters: SURVEY.md Appendix A, each from the cited species file."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .. import _lib
from ..dichromat import AutoNight, DichromatOp, DichromatSpec, NightSpec, as_fov
from .animal import Animal
from .animal_utils import check_input_image


class _Dichromat(Animal):
    SPEC: DichromatSpec = None  # type: ignore

    def __init__(self, *, night=None, fov=None):
        """fov: None, or a FovSpec (or its arguments as a tuple): visualize(uint8) then returns (centre-zoomed input, wide view) --
        the reference's binocular warp in front of this species' colour stage, the pair Cat returns.
        night: None (by day, the reference's active code), True (NightSpec's defaults: the values of the commented night
        branch of animals/cat.py:50-60) or a NightSpec: rod vision in front of the colour stage, optional tapetum bloom; or an
        AutoNight: every frame by day or as its NightSpec says, decided by the frame's median luma."""
        self._op = None
        if night is True:
            night = NightSpec()
        elif night is False:
            night = None
        if night is not None and not isinstance(night, (NightSpec, AutoNight)):
            raise TypeError(f"night must be None, True, a NightSpec or an AutoNight (got {type(night).__name__})")
        self.night = night
        self.fov = as_fov(fov)

    def _operator(self) -> DichromatOp:
        if self._op is None:
            self._op = DichromatOp(self.SPEC, night=self.night)
        return self._op

    def _refuse_float_night(self, image: np.ndarray) -> None:
        if self.night is not None and image.dtype != np.uint8:
            what = "night=AutoNight" if isinstance(self.night, AutoNight) else "night"
            raise NotImplementedError(f"{type(self).__name__}: {what} is implemented for uint8 frames, got {image.dtype}")

    def _refuse_float_fov(self, image: np.ndarray) -> None:
        if self.fov is not None and image.dtype != np.uint8:
            raise NotImplementedError(f"{type(self).__name__}: fov is implemented for uint8 frames, got {image.dtype}")

    def _fov_constants(self):
        """(camera_hfov_deg, per_eye_half_fov_deg, overlap_deg, to_human_ratio) of the wide view."""
        f = self.fov
        return f.camera_hfov_deg, f.per_eye_half_fov_deg, f.overlap_deg, f.to_human_ratio

    def _visualize_wide_u8(self, image: np.ndarray):
        """One uint8 frame through the stream operator's launches (WideStreamOp): device tables and buffers are kept per size."""
        H, W = image.shape[:2]
        plans = self.__dict__.setdefault("_u8_plans", {})
        key = (H, W, bool(getattr(self, "ENABLE_FOV_WARP", True)), *self._fov_constants(), self.night)
        sop = plans.get(key)
        if sop is None:
            if len(plans) >= 4:
                plans.pop(next(iter(plans))).close()
            sop = plans[key] = (CatStreamOp if isinstance(self, Cat) else WideStreamOp)(self, H, W, depth=1, batch=1)
        ctx = sop.ctx
        d_in, d_out = sop.slot_buffers(0)
        ctx.upload(image, d_in)
        sop.run_device(d_in, d_out, 1, H, W)
        wide = ctx.download(d_out, image.shape, np.uint8)
        d_base = sop.slot_baseline(0)
        zoomed = image if d_base is d_in else ctx.download(d_base, image.shape, np.uint8)  # center_zoom at scale <= 1: the frame itself
        return zoomed, wide

    def visualize(self, image: np.ndarray) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        assert check_input_image(image)  # dog.py:33
        self._refuse_float_night(image)
        self._refuse_float_fov(image)
        if self.fov is not None:
            return self._visualize_wide_u8(image)
        if image.dtype != np.uint8:
            # The reference tolerates float / wider-int frames (animal_utils.py:45-48); its video, webcam and image
            # renderers only ever produce uint8 (video.py:95).  Float frames of the Gaussian / row-gain species run as a
            # plane program; anything else is not silently re-routed to a CPU path: say so.
            if np.issubdtype(image.dtype, np.floating) and self.SPEC.color == "collapse":
                return image, self._visualize_float(image)
            raise NotImplementedError(f"{type(self).__name__}: device path implemented for uint8 frames (and float frames of the "
                                      f"collapse-matrix species), got {image.dtype}")
        return image, self._operator()(image)

    def _visualize_float(self, image: np.ndarray) -> np.ndarray:
        """dog.py:37-59 for a float frame: get_normalized_image's `max > 1` rule (a frame-wide reduction), both transfer
        functions as expressions, `px @ T.T`, cv2.GaussianBlur((0,0), sigma) or the S-cone row gain; float32 sRGB out."""
        from ..dichromat import collapse_LMS_matrix, cv_auto_ksize, gaussian_taps, s_cone_row_gain
        from ..planevm import DeviceBackend, PlaneRef

        plans = self.__dict__.setdefault("_float_plans", {})
        key = image.shape[:2]
        be = plans.get(key)
        if be is None:
            if len(plans) >= 4:
                plans.pop(next(iter(plans))).close()
            H, W = key
            sp = self.SPEC
            be = DeviceBackend(H, W, float_frames=True)
            y = [be.load(PlaneRef(be.d_in, 4 * c, 3)) for c in range(3)]
            mx = be.max(be.maximum(be.maximum(y[0], y[1]), y[2]))
            a = 0.055
            lin = []
            for c in range(3):  # get_normalized_image (animal_utils.py:41-50) + srgb_to_linear (:5-11)
                x = be.clip01(be.where(mx > 1.0, y[c] / 255.0, y[c]))
                lin.append(be.where(x <= 0.04045, x / 12.92, ((x + a) / (1 + a)) ** 2.4))
            T = collapse_LMS_matrix(sp.alpha, sp.s_scale)  # float32 3x3; out_i = sum_j T[i][j] * in_j (dog.py:47)
            rgb = [lin[0] * float(T[i, 0]) + lin[1] * float(T[i, 1]) + lin[2] * float(T[i, 2]) for i in range(3)]
            if sp.post == "gauss":
                k = cv_auto_ksize(sp.sigma)
                rgb = be.blur_taps(rgb, k, gaussian_taps(k, sp.sigma))
            elif sp.post == "scone":
                s_top, s_bottom, power, boost = sp.scone
                rgb = [rgb[0], rgb[1], be.clip01(rgb[2] * be.row(s_cone_row_gain(H, s_top, s_bottom, power=power, extra_boost=boost)))]
            elif sp.post == "streak":  # animal_utils.py:147-172 as coded (Q3); the float32 frame is blurred in place (Q4)
                rgb = be.streak(rgb, sp.streak)
            if sp.chroma is not None:  # apply_chroma_compression (animal_utils.py:174-181), where its result is used
                gray = ((rgb[0] + rgb[1]) + rgb[2]) / 3.0
                keep = float(np.float32(1.0 - sp.chroma))
                rgb = [gray + (v - gray) * keep for v in rgb]
            for c in range(3):  # np.clip(linear_to_srgb(np.clip(x, 0, 1)), 0, 1).astype(dtype)  (dog.py:54-59)
                x = be.clip01(rgb[c])
                be.store(be.clip01(be.where(x <= 0.0031308, 12.92 * x, (1 + a) * be.power(x, 1 / 2.4) - a)), PlaneRef(be.d_out, 4 * c, 3))
            be.flush()
            plans[key] = be
        ctx = be.ctx
        ctx.upload(np.ascontiguousarray(image, dtype=np.float32), be.d_in)
        be.run_device()
        out = ctx.download(be.d_out, image.shape, np.float32)
        return out.astype(image.dtype, copy=False)


def _mk(cls_name: str, spec: DichromatSpec, doc: str):
    return type(cls_name, (_Dichromat,), {"SPEC": spec, "__doc__": doc})


Dog = _mk("Dog", DichromatSpec("dog", 0.58, 0.65, sigma=3.5), "animals/dog.py:46,51")
Squirrel = _mk("Squirrel", DichromatSpec("squirrel", 0.55, 1.05, sigma=0.7), "animals/squirrel.py:29,34")
Elephant = _mk("Elephant", DichromatSpec("elephant", 0.60, 0.95, sigma=1.8), "animals/elephant.py:29,34")
Lion = _mk("Lion", DichromatSpec("lion", 0.60, 0.95, sigma=1.2), "animals/lion.py:29,34")
Tiger = _mk("Tiger", DichromatSpec("tiger", 0.60, 0.95, sigma=1.2), "animals/tiger.py:29,34")
Bear = _mk("Bear", DichromatSpec("bear", 0.60, 0.95, sigma=1.6), "animals/bear.py:29,34")
Wolf = _mk("Wolf", DichromatSpec("wolf", 0.65, 0.95, sigma=1.4), "animals/wolf.py:29,34")
Fox = _mk("Fox", DichromatSpec("fox", 0.65, 0.98, sigma=1.3), "animals/fox.py:29,34")
Raccoon = _mk("Raccoon", DichromatSpec("raccoon", 0.60, 0.98, sigma=2.0), "animals/raccoon.py:29,34")
Rat = _mk("Rat", DichromatSpec("rat", 0.05, 0.86, post="scone", scone=(1.3, 0.5, 1.4, 0.25)), "animals/rat.py:29,34")
# Streak-blur species: apply_anisotropic_acuity_blur_with_streak as coded (quirks Q3/Q4), csrc/dichromat_streak.hip.
Sheep = _mk("Sheep", DichromatSpec("sheep", 0.74, 1.06, post="streak", streak=(0.48, 0.8, 2.2, 6.0)), "animals/sheep.py:30,35")
Pig = _mk("Pig", DichromatSpec("pig", 0.89, 1.32, post="streak", streak=(0.5, 1.2, 2.5, 3.0)), "animals/pig.py:30,35,38 (chroma result discarded, Q4)")
Cow = _mk("Cow", DichromatSpec("cow", 0.84, 1.07, post="streak", streak=(0.5, 0.9, 2.3, 6.5)), "animals/cow.py:29,34")
Goat = _mk("Goat", DichromatSpec("goat", 0.75, 1.06, post="streak", streak=(0.5, 0.8, 2.4, 8.0)), "animals/goat.py:29,34")
Horse = _mk("Horse", DichromatSpec("horse", 0.30, 1.02, post="streak", streak=(0.5, 0.8, 2.2, 6.0)), "animals/horse.py:29,34")
Rabbit = _mk("Rabbit", DichromatSpec("rabbit", 0.20, 1.01, post="streak", streak=(0.52, 0.9, 2.5, 5.0), chroma=0.06), "animals/rabbit.py:29,34,37")
Panda = _mk("Panda", DichromatSpec("panda", 0.58, 0.74, post="streak", streak=(0.52, 1.0, 2.1, 4.5), chroma=0.06), "animals/panda.py:29,34,37")
Deer = _mk("Deer", DichromatSpec("deer", 0.60, 0.95, post="streak", streak=(0.5, 0.8, 2.6, 8.0)), "animals/deer.py:29,34")
Kangaroo = _mk("Kangaroo", DichromatSpec("kangaroo", 0.60, 0.98, post="streak", streak=(0.55, 0.8, 2.3, 8.0)), "animals/kangaroo.py:29,34")


class Cat(_Dichromat):
    """animals/cat.py (Tina-animals side of the unresolved merge, quirk Q8): returns (human_zoomed, cat_wide).

    human_zoomed = centre zoom of the input (cat.py:74-79, uint8 INTER_LINEAR); cat_wide = binocular wide-FOV
    warp of the ORIGINAL (cat.py:82-92) -> float64 L/M-merge colour tail -> sigma 1.0 blur -> OETF (cat.py:95-109).
    With ENABLE_FOV_WARP the warp output is float, so its sRGB decode uses the device powf (final bytes within
    1 code of the reference); with it off the uint8 path is bit-exact."""

    SPEC = DichromatSpec("cat", 0.5, 1.0, color="cat_merge", sigma=1.0)
    CAMERA_HFOV_DEG = 100.0
    CAT_PER_EYE_HALF_FOV_DEG = 105.0
    CAT_OVERLAP_DEG = 40.0
    CAT_TO_HUMAN_RATIO = 1.30
    ENABLE_FOV_WARP = True

    def __init__(self, *, night=None, fov=None):
        """fov: a FovSpec (or its arguments as a tuple) sets this instance's four FOV constants; every route follows them."""
        super().__init__(night=night, fov=fov)
        if self.fov is not None:
            self.CAMERA_HFOV_DEG, self.CAT_PER_EYE_HALF_FOV_DEG = float(self.fov.camera_hfov_deg), float(self.fov.per_eye_half_fov_deg)
            self.CAT_OVERLAP_DEG, self.CAT_TO_HUMAN_RATIO = float(self.fov.overlap_deg), float(self.fov.to_human_ratio)

    def _fov_constants(self):
        return self.CAMERA_HFOV_DEG, self.CAT_PER_EYE_HALF_FOV_DEG, self.CAT_OVERLAP_DEG, self.CAT_TO_HUMAN_RATIO

    def visualize(self, image: np.ndarray):
        assert isinstance(image, np.ndarray) and image.ndim == 3 and image.shape[2] == 3, "HxWx3 RGB"
        self._refuse_float_night(image)
        if image.dtype != np.uint8:
            if np.issubdtype(image.dtype, np.floating):
                return self._visualize_float(image)
            raise NotImplementedError(f"Cat: device path implemented for uint8 and float frames, got {image.dtype}")
        return self._visualize_wide_u8(image)

    def _visualize_float(self, image: np.ndarray):
        """cat.py:73-112 for a float frame, as a plane program in float32 (the reference's float64 tail is held to the float
        pipeline's 1e-4, like every float frame): get_normalized_image's `max > 1` rule, the binocular warp as two
        cv2.remap's with per-column / per-row maps + the cos^2 blend, srgb_to_linear, RGB->LMS, L/M merge, LMS->RGB, sigma 1.0
        blur, OETF; returns (centre-zoomed input, cat view), both in the input's dtype."""
        from .. import geometry as G
        from ..dichromat import cv_auto_ksize, gaussian_taps
        from ..planevm import DeviceBackend, PlaneRef

        H, W = image.shape[:2]
        scale = G.zoom_scale_from_cat_ratio(camera_hfov_deg=self.CAMERA_HFOV_DEG, cat_per_eye_half_fov_deg=self.CAT_PER_EYE_HALF_FOV_DEG,
                                            cat_to_human_ratio=self.CAT_TO_HUMAN_RATIO)
        human_zoomed = G.center_zoom(image, scale=scale)
        plans = self.__dict__.setdefault("_float_plans", {})
        key = (H, W, bool(self.ENABLE_FOV_WARP))
        be = plans.get(key)
        if be is None:
            if len(plans) >= 4:
                plans.pop(next(iter(plans))).close()
            be = DeviceBackend(H, W, float_frames=True)
            y = [be.load(PlaneRef(be.d_in, 4 * c, 3)) for c in range(3)]
            mx = be.max(be.maximum(be.maximum(y[0], y[1]), y[2]))
            x = [be.clip01(be.where(mx > 1.0, v / 255.0, v)) for v in y]  # get_normalized_image (animal_utils.py:41-50)
            if self.ENABLE_FOV_WARP:  # cat_widevision_utils.py:46-99
                xL, xR, ymap, wL, wR = G.binocular_warp_tables(H, W, W, H, self.CAMERA_HFOV_DEG, self.CAT_PER_EYE_HALF_FOV_DEG, self.CAT_OVERLAP_DEG)
                my = be.row(ymap)
                left = be.remap(x, be.col(xL), my, 0.0)
                right = be.remap(x, be.col(xR), my, 0.0)
                cwl, cwr = be.col(wL), be.col(wR)
                wsum = cwl + cwr + 1e-8
                x = [be.clip01((left[c] * cwl + right[c] * cwr) / wsum) for c in range(3)]
            a = 0.055
            lin = [be.where(v <= 0.04045, v / 12.92, ((v + a) / (1 + a)) ** 2.4) for v in x]
            M = [[0.31399022, 0.63951294, 0.04649755], [0.15537241, 0.75789446, 0.08670142], [0.01775239, 0.10944209, 0.87256922]]
            Bk = [[5.472213, -4.6419606, 0.16963711], [-1.125242, 2.2931712, -0.16789523], [0.02980164, -0.19318072, 1.1636479]]
            lms = [lin[0] * M[i][0] + lin[1] * M[i][1] + lin[2] * M[i][2] for i in range(3)]       # animal_utils.py:52-63
            al = float(np.float32(self.SPEC.alpha))
            lm = lms[0] * al + lms[1] * float(np.float32(1.0 - self.SPEC.alpha))                    # cat.py:99
            rgb = [lm * Bk[i][0] + lm * Bk[i][1] + lms[2] * Bk[i][2] for i in range(3)]            # LMS_to_RGB (:65-77)
            k = cv_auto_ksize(self.SPEC.sigma)
            rgb = be.blur_taps(rgb, k, gaussian_taps(k, self.SPEC.sigma))
            for c in range(3):
                v = be.clip01(rgb[c])
                be.store(be.clip01(be.where(v <= 0.0031308, 12.92 * v, (1 + a) * be.power(v, 1 / 2.4) - a)), PlaneRef(be.d_out, 4 * c, 3))
            be.flush()
            plans[key] = be
        ctx = be.ctx
        ctx.upload(np.ascontiguousarray(image, dtype=np.float32), be.d_in)
        be.run_device()
        out = ctx.download(be.d_out, image.shape, np.float32)
        return human_zoomed.astype(image.dtype, copy=False), out.astype(image.dtype, copy=False)


class WideStreamOp:
    """The wide view of a dichromat as a frame-loop operator (pipeline.FramePipeline's protocol, like SpeciesStreamOp): Cat, or any of
    the 19 other dichromats built with fov=.  Per slot `batch` contiguous uint8 frames in, out and baseline on the
    device; once per op the five binocular warp tables.  run_device enqueues two launches on the slot's stream: avx_center_zoom_u8
    into the slot's baseline (visualize()'s first frame, the split frame's left half) and the fused wide view -- avx_cat_wide_u8 for
    Cat, avx_dichromat_wide_u8 for the others (csrc/dichromat_wide.hip: warp, colour stage, post stage and encode behind
    one entry).  With Cat's ENABLE_FOV_WARP false the wide view is the ordinary dichromat kernel on the uint8 frames; with a zoom
    scale <= 1 the baseline is the input itself.  The buffers are plain allocations of the op, which outlive the slot streams.
    At night (night=...) the wide view is the chain the fused kernel is defined by, with the night entry at its
    end: avx_binocular_warp_u8 per frame into the slot's float32 frames, then avx_dichromat_night_u8 with in_f32 = 1 on the batch;
    with ENABLE_FOV_WARP false the night entry on the uint8 frames.  The baseline launch is the same.
    With night=AutoNight(...) the decision is taken on the slot's input frames -- the scene, not the warp:
    avx_luma_mode_u8, the records into pinned memory, one synchronisation of the slot's stream -- and the batch is walked in runs
    of equal mode: a day run is one fused launch, a night run the chain above; with ENABLE_FOV_WARP false the
    switched entry avx_dichromat_auto_u8 does the same inside the library.  `last_modes` and `auto_counts` as DichromatOp's."""

    def __init__(self, animal: _Dichromat, H: int, W: int, depth: int = 3, batch: int = 1, ctx=None):
        from .. import geometry as G

        if batch < 1:
            raise ValueError(f"batch must be at least 1 (got {batch})")
        self.animal = self.cat = animal
        self.H, self.W = int(H), int(W)
        self.batch = self.max_batch = int(batch)
        self._op = animal._operator() if ctx is None else DichromatOp(animal.SPEC, ctx, night=animal.night)
        self.ctx = self._op._ctx()
        self.warp = bool(getattr(animal, "ENABLE_FOV_WARP", True))
        self.rect = self.crop_rect(animal, self.H, self.W)
        camera, phi, overlap, _ = animal._fov_constants()
        nbytes = self.batch * self.H * self.W * 3
        self._bufs = [(self.ctx.malloc(nbytes), self.ctx.malloc(nbytes)) for _ in range(depth)]
        self._base = [self.ctx.malloc(nbytes) if self.rect is not None else None for _ in range(depth)]
        self._by_in = {d_in.ptr: k for k, (d_in, _) in enumerate(self._bufs)}
        self._tables, self._table_ptrs = None, None
        self.night = animal.night
        self.auto = animal.night if isinstance(animal.night, AutoNight) else None
        self.last_modes, self.auto_counts = np.zeros(0, np.uint8), [0, 0]
        self._warped, self._host_tables, self._op_f32 = [], None, None
        self._rec, self._rec_host = None, None
        self._wide_day = G.cat_wide_device if isinstance(animal, Cat) else G.dichromat_wide_device
        if self.warp and self.auto is not None:
            self._rec = self.ctx.malloc(16 * 16)
            self._rec_host = self.ctx.pinned((16,), _lib.LUMA_MODE_REC_DTYPE)
        if self.warp and self.night is not None:
            self._host_tables = G.binocular_warp_tables(self.H, self.W, self.W, self.H, camera, phi, overlap)
            self._warped = [self.ctx.malloc(nbytes * 4) for _ in range(depth)]  # float32 HWC frames in [0, 1]
            self._op_f32 = DichromatOp(animal.SPEC, self.ctx, night=self.auto.night if self.auto is not None else self.night)
            self._op_f32.desc.in_f32 = 1
        if self.warp and (self.night is None or self.auto is not None):
            tables = G.binocular_warp_tables(self.H, self.W, self.W, self.H, camera, phi, overlap)
            self._tables, self._table_ptrs = G.binocular_warp_tables_device(self.ctx, tables)

    @staticmethod
    def crop_rect(animal, H: int, W: int):
        """The crop (x0, y0, cw, ch) of the H x W frame that the baseline enlarges (cat.py:74-79), or None at a zoom scale <= 1:
        the baseline is the input.  Host arithmetic only."""
        from .. import geometry as G

        camera, phi, _, ratio = animal._fov_constants()
        scale = G.zoom_scale_from_cat_ratio(camera_hfov_deg=camera, cat_per_eye_half_fov_deg=phi, cat_to_human_ratio=ratio)
        return G.center_zoom_rect(H, W, scale)

    def slot_buffers(self, k: int):
        return self._bufs[k]

    def slot_baseline(self, k: int):
        """Slot k's baseline frames (uint8, on the device): the centre-zoomed input, or the slot's input at a zoom scale <= 1."""
        return self._base[k] if self.rect is not None else self._bufs[k][0]

    def run_device(self, d_in, d_out, n_frames: int, H: int, W: int, stream=None):
        from .. import geometry as G

        assert 1 <= n_frames <= self.batch and (H, W) == (self.H, self.W)
        if self._table_ptrs is not None:  # the day desc's per-row host tables: the species' op is shared by its operators of every size
            self._op.prepare_tables(H)
        if self.rect is not None:
            G.center_zoom_device(self.ctx, d_in, self._base[self._by_in[d_in.ptr]], n_frames, H, W, self.rect, stream)
        if self.warp and self.auto is not None:
            from ..dichromat import finish_modes, luma_records_device

            rec = luma_records_device(self.ctx, d_in.ptr, n_frames, H, W, self.auto.threshold, self._rec, out=self._rec_host.array, stream=stream)
            modes = finish_modes(rec["below"], rec["max_below"], rec["min_at_or_above"], H * W, self.auto.threshold).astype(np.uint8)
            fb, f0 = H * W * 3, 0
            while f0 < n_frames:
                f1 = f0 + 1
                while f1 < n_frames and modes[f1] == modes[f0]:
                    f1 += 1
                run_in, run_out = d_in.view(f0 * fb, (f1 - f0) * fb), d_out.view(f0 * fb, (f1 - f0) * fb)
                if modes[f0]:
                    self._wide_night(run_in, run_out, self._warped[self._by_in[d_in.ptr]], f1 - f0, H, W, stream)
                else:
                    self._wide_day(self.ctx, run_in, run_out, f1 - f0, H, W, self._op.desc, self._table_ptrs, stream)
                f0 = f1
            self._note_modes(modes)
        elif self.warp and self.night is not None:
            self._wide_night(d_in, d_out, self._warped[self._by_in[d_in.ptr]], n_frames, H, W, stream)
        elif self.warp:
            self._wide_day(self.ctx, d_in, d_out, n_frames, H, W, self._op.desc, self._table_ptrs, stream)
        else:
            self._op.run_device(d_in, d_out, n_frames, H, W, stream=stream)
            if self.auto is not None:
                self._note_modes(self._op.last_modes)

    def _note_modes(self, modes: np.ndarray) -> None:
        self.last_modes = np.array(modes, np.uint8)
        self.auto_counts[0] += int(self.last_modes.sum())
        self.auto_counts[1] += self.last_modes.size

    def _wide_night(self, d_in, d_out, d_f32, n_frames: int, H: int, W: int, stream) -> None:
        """The night chain on n_frames frames: the binocular warp per frame into d_f32's first frames, then the night entry."""
        xL, xR, ymap, wL, wR = self._host_tables
        for f in range(n_frames):
            self.ctx._check(_lib.lib.avx_binocular_warp_u8(self.ctx._h, d_in.ptr + f * H * W * 3, H, W, xL.ctypes.data, xR.ctypes.data, ymap.ctypes.data,
                                                           wL.ctypes.data, wR.ctypes.data, H, W, d_f32.ptr + f * H * W * 12, self.ctx._s(stream)))
        self._op_f32.run_device(d_f32, d_out, n_frames, H, W, stream=stream)

    def close(self):
        for pair in self._bufs:
            for b in pair:
                b.free()
        for b in self._base + [self._tables, self._rec, self._rec_host] + self._warped:
            if b is not None:
                b.free()
        self._bufs, self._base, self._tables, self._warped, self._rec, self._rec_host = [], [], None, [], None, None


class CatStreamOp(WideStreamOp):
    """WideStreamOp for Cat, whose geometry is its four FOV constants: the wide view goes through avx_cat_wide_u8."""
