"""CPU-only: the restatement of the marching kernel's strip / chunk formulas (tests/_march_geometry.py) against values
computed by hand from csrc/dichromat_march.hip, and the sigma -> radius choices the geometry sweep relies on."""
import _march_geometry as G

from animal_vision_amd import dichromat as D


def test_chunk_formula_hand_values():
    # H = 1080, 8 chunks: ceil(1080 / 8) = 135 -> 136 rows (multiple of 4); 7 * 136 = 952, the 8th chunk has 128
    assert G.set_chunks(1080, 8) == (8, 136) and G.last_chunk_rows(1080, 8, 136) == 128
    # H = 1057, 24 chunks: ceil(1057 / 24) = 45 -> 48 rows; 22 * 48 = 1056, the 23rd chunk has 1 row
    assert G.set_chunks(1057, 24) == (23, 48) and G.last_chunk_rows(1057, 23, 48) == 1
    assert G.set_chunks(1059, 24) == (23, 48) and G.last_chunk_rows(1059, 23, 48) == 3
    assert G.set_chunks(1061, 24) == (23, 48) and G.last_chunk_rows(1061, 23, 48) == 5
    # requests are clamped to H // 32 chunks: 1080 // 32 = 33 -> ceil(1080 / 33) = 33 -> 36 rows, 30 chunks
    assert G.set_chunks(1080, 10**6) == G.set_chunks(1080, 33) == (30, 36)
    assert G.set_chunks(36, 24) == (1, 36) and G.set_chunks(20, 3) == (1, 20)  # H // 32 == 1 / == 0: one chunk
    assert G.set_chunks(2160, 3) == (3, 720)


def test_strip_formula_hand_values():
    # W = 1921 under a 128-px cap: 16 strips; ceil(1921 / 16) = 121 -> 122 -> 128 (16-px multiple fits the cap): 15 * 128 = 1920, last 1 px
    assert G.set_strips(1921, 128, 2) == (16, 128) and G.last_strip_px(1921, 16, 128) == 1
    # the same frame with 384-thread workgroups (256-px cap): 8 strips of 256, the last 129 px
    assert G.set_strips(1921, 256, 2) == (8, 256) and G.last_strip_px(1921, 8, 256) == 129
    # 1080p: 15 strips of 128; narrowed (112-px cap): 18 strips; ceil(1920 / 18) = 107 -> 108 -> 112
    assert G.set_strips(1920, 128, 2) == (15, 128)
    assert G.set_strips(1920, 112, 2) == (18, 112) and G.last_strip_px(1920, 18, 112) == 16
    # the cat's 120-px cap: W = 354 -> 3 strips of 118 (128 would not fit the cap)
    assert G.set_strips(354, 120, 2) == (3, 118) and G.last_strip_px(354, 3, 118) == 118
    assert G.set_strips(1920, 120, 2) == (16, 120)
    # 4 columns per thread (R = 1, 3): 256-px strips; 3841 = 15 * 256 + 1
    assert G.set_strips(3841, 256, 4) == (16, 256) and G.last_strip_px(3841, 16, 256) == 1
    assert G.set_strips(52, 128, 2) == (1, 64)  # narrower than one strip


def test_instantiation_table_and_narrowed_widths():
    assert G.march_cfg(14, False, 64) == (2, 128, 128, True) and G.march_cfg(14, False, 128) == (2, 256, 256, False)
    assert G.march_cfg(3, False, 64) == (4, 256, 256, True) and G.march_cfg(1, False, 128) == (4, 512, 512, False)
    assert G.march_cfg(4, True, 64) == (2, 128, 120, True) and G.march_cfg(4, True, 128) == (2, 256, 256, False)
    # launch_march's sw_narrow: 240 px for R = 1, 3; 112 px for R = 4..8; 96 px for R = 9, 14; none for float64 / NG = 128
    assert [G.narrowed_width(R, False, 64) for R in (1, 3, 4, 5, 6, 7, 8, 9, 14)] == [240, 240, 112, 112, 112, 112, 112, 96, 96]
    assert G.narrowed_width(4, True, 64) == 0 and all(G.narrowed_width(R, False, 128) == 0 for R in (1, 3, 6, 14))


def test_expected_launch_and_xcd_remap():
    e = G.expected_launch(6, False, 64, 1, 1080, 1920, 8)
    assert (e["nstrips"], e["sw"], e["nchunks"], e["ch"], e["grid"], e["xcd_remap"], e["spec"]) == (15, 128, 8, 136, 120, 1, 1)
    e = G.expected_launch(6, False, 64, 1, 1080, 1920, 3, narrow=True)
    assert (e["nstrips"], e["sw"], e["nchunks"], e["ch"], e["grid"], e["xcd_remap"], e["narrow"]) == (18, 112, 3, 360, 54, 0, 1)
    e = G.expected_launch(14, False, 128, 1, 720, 1280, 1)
    assert (e["nstrips"], e["sw"], e["grid"], e["xcd_remap"], e["spec"]) == (5, 256, 5, 0, 0)


def test_sigmas_that_reach_the_radius_1_and_9_instantiations():
    """No species has R = 1 or R = 9; the sweep reaches those kernels through dataclasses.replace(spec, sigma=...)."""
    assert D.cv_auto_ksize(0.3) == 3 and D.cv_auto_ksize(2.25) == 19
    radii = {n: D.cv_auto_ksize(s) // 2 for n, s in (("squirrel", 0.7), ("cat", 1.0), ("lion", 1.2), ("wolf", 1.4), ("bear", 1.6), ("raccoon", 2.0), ("dog", 3.5))}
    assert radii == {"squirrel": 3, "cat": 4, "lion": 5, "wolf": 6, "bear": 7, "raccoon": 8, "dog": 14}
