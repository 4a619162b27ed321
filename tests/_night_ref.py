"""The night form of the dichromats, composed from oracle.cpu_ref functions (tests only).

Per uint8 frame and species spec `sp` (cpu_ref.DICHROMATS[...]), with rod = (chroma_scale, luminance_boost, gamma) and bloom
strength S:
  1. lin = srgb_to_linear(get_normalized_image(image))      -- Cat with the warp: animal_fov_binocular_warp first (cat_visualize)
  2. lin = apply_rod_vision(lin, *rod)
  3. colour stage, post stage, chroma compression            -- exactly dichromat_visualize's lines (Pig's quirks included)
  4. S > 0: rgb = apply_tapetum_bloom(rgb, S, 3.0)
  5. encode_u8
`jit` (cpu_ref.relative_jitter(seed)) is applied to the result of each of the steps 1-4: the sensitivity probe of tests/_sensitivity."""
import numpy as np

from oracle import cpu_ref

ROD_DEFAULT = (0.07, 1.8, 0.7)


def frames(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    """The uint8 test frames of the night tests."""
    rng = np.random.default_rng(1000 + seed)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "noise":
        return noise
    if kind == "dark":
        return noise // 6
    if kind == "ramp":
        x = np.linspace(0, 255, W)[None, :, None]
        y = np.linspace(0, 1, H)[:, None, None]
        return np.clip(np.concatenate([x * y, x * (1 - y), x * np.ones_like(y)], axis=2), 0, 255).astype(np.uint8)
    if kind == "lamps":  # a dim scene with three saturated discs, one cut by a corner
        f = noise // 8
        yy, xx = np.mgrid[0:H, 0:W]
        r = max(3, min(H, W) // 6)
        for cy, cx in ((0, 0), (H // 2, W // 2), (H - 1 - r, W // 4)):
            f[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
        return f
    if kind == "white":
        return np.full((H, W, 3), 255, np.uint8)
    if kind == "black":
        return np.zeros((H, W, 3), np.uint8)
    if kind == "ones":  # every byte 0 or 1: get_normalized_image does not divide by 255
        return (noise & 1).astype(np.uint8)
    raise ValueError(kind)


def night_lin(sp, image: np.ndarray, *, rod=ROD_DEFAULT, bloom: float = 0.0, jit=None, cat_warp: bool = True) -> np.ndarray:
    """Steps 1-4: the linear frame that encode_u8 receives."""
    j = (lambda a: a) if jit is None else jit
    assert cpu_ref.check_input_image(image) and image.dtype == np.uint8
    x01 = cpu_ref.get_normalized_image(image)
    if sp.name == "cat" and cat_warp:  # cat_visualize, cpu_ref.py:1073-1077
        H, W = image.shape[:2]
        x01 = cpu_ref.animal_fov_binocular_warp(x01.astype(np.float32), fov_in_deg=100.0, per_eye_half_fov_deg=105.0, overlap_deg=40.0,
                                                out_size=(W, H), border_value=0.0)
    lin = j(cpu_ref.srgb_to_linear(x01))
    lin = j(cpu_ref.apply_rod_vision(lin, *rod))
    rgb = cpu_ref.dichromat_color_stage(sp, lin)  # dichromat_visualize, cpu_ref.py:378-391
    if sp.post == "gauss":
        rgb = cpu_ref.apply_acuity_blur(rgb, sp.sigma)
    elif sp.post == "streak":
        r = cpu_ref.apply_anisotropic_acuity_blur_with_streak(rgb, *sp.streak)
        if not sp.streak_result_discarded:
            rgb = r
    elif sp.post == "scone":
        s_top, s_bottom, power, boost = sp.scone
        rgb = cpu_ref.apply_s_cone_vertical_gain(rgb, s_top=s_top, s_bottom=s_bottom, power=power, extra_boost=boost)
    if sp.chroma is not None:
        c = cpu_ref.apply_chroma_compression(rgb, sp.chroma)
        if not sp.chroma_discarded:
            rgb = c
    rgb = j(rgb)
    if bloom > 0:
        rgb = j(cpu_ref.apply_tapetum_bloom(rgb, bloom, 3.0))
    return rgb


def night_ref(sp, image: np.ndarray, *, rod=ROD_DEFAULT, bloom: float = 0.0, jit=None, cat_warp: bool = True) -> np.ndarray:
    """The oracle's night frame (uint8)."""
    return cpu_ref.encode_u8(night_lin(sp, image, rod=rod, bloom=bloom, jit=jit, cat_warp=cat_warp), np.uint8)


def cat_baseline(image: np.ndarray) -> np.ndarray:
    """visualize()'s first frame for Cat: the centre-zoomed input, by night as by day (cat_visualize)."""
    scale = cpu_ref.zoom_scale_from_cat_ratio(camera_hfov_deg=100.0, cat_per_eye_half_fov_deg=105.0, cat_to_human_ratio=1.30)
    return cpu_ref.center_zoom(image, scale=scale)
