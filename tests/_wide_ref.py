"""The wide view of the dichromats, composed from oracle.cpu_ref functions (tests only).

Per uint8 frame, species spec `sp` (cpu_ref.DICHROMATS[...]) and geometry (phi, O, camera):
  1. x01 = animal_fov_binocular_warp(get_normalized_image(image).astype(float32), fov_in_deg = camera, per_eye_half_fov_deg = phi,
           overlap_deg = O, out_size = (W, H))                     -- cat_visualize's call, cpu_ref.py:1073-1076, with the geometry open
  2. lin = srgb_to_linear(x01)
  3. rod = (chroma_scale, luminance_boost, gamma): lin = apply_rod_vision(lin, *rod)
  4. colour stage, post stage, chroma compression                   -- exactly dichromat_visualize's lines 379-391 (Pig's quirks included)
  5. bloom > 0: rgb = apply_tapetum_bloom(rgb, bloom, 3.0)
  6. encode_u8
`jit` (cpu_ref.relative_jitter(seed)) is applied to the result of each of the steps 2-5: the sensitivity probe of tests/_sensitivity.
The baseline is center_zoom(image, zoom_scale_from_cat_ratio(camera, phi, ratio))."""
import numpy as np

from oracle import cpu_ref

# (phi, O, camera): Cat's (about 30 % black columns, one eye elsewhere); about 60 % black columns; no black column and both eyes
# fetched on most columns -- the only one that exercises the two-eye blend
GEOMETRIES = [(105.0, 40.0, 100.0), (100.0, 20.0, 60.0), (50.0, 80.0, 100.0)]
CAT_GEOMETRY, NARROW_CAMERA, TWO_EYES = GEOMETRIES
ROD_DEFAULT = (0.07, 1.8, 0.7)


def wide_lin(sp, image: np.ndarray, geometry, *, rod=None, bloom: float = 0.0, jit=None) -> np.ndarray:
    """Steps 1-5: the linear frame that encode_u8 receives."""
    j = (lambda a: a) if jit is None else jit
    assert cpu_ref.check_input_image(image) and image.dtype == np.uint8
    phi, overlap, camera = geometry
    H, W = image.shape[:2]
    x01 = cpu_ref.animal_fov_binocular_warp(cpu_ref.get_normalized_image(image).astype(np.float32), fov_in_deg=camera, per_eye_half_fov_deg=phi,
                                            overlap_deg=overlap, out_size=(W, H))
    lin = j(cpu_ref.srgb_to_linear(x01))
    if rod is not None:
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


def wide_ref(sp, image: np.ndarray, geometry, *, rod=None, bloom: float = 0.0, jit=None) -> np.ndarray:
    """The oracle's wide view (uint8)."""
    return cpu_ref.encode_u8(wide_lin(sp, image, geometry, rod=rod, bloom=bloom, jit=jit), np.uint8)


def baseline(image: np.ndarray, geometry, ratio: float = 1.30) -> np.ndarray:
    """visualize()'s first frame with a field of view: the centre-zoomed input."""
    phi, _, camera = geometry
    scale = cpu_ref.zoom_scale_from_cat_ratio(camera_hfov_deg=camera, cat_per_eye_half_fov_deg=phi, cat_to_human_ratio=ratio)
    return cpu_ref.center_zoom(image, scale=scale)


def lit_columns(W: int, geometry) -> np.ndarray:
    """bool[W]: the output columns for which at least one eye looks into the camera's frame."""
    phi, overlap, camera = geometry
    _, _, _, wL, wR = cpu_ref.binocular_warp_maps(4, W, W, 4, camera, phi, overlap)
    return (wL[0] + wR[0]) > 0
