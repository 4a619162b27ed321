"""The gallery command's host side (reference: gallery_grid.py:8-106, main.py:98-139 / :163-278, utils.py:91-130): layout numbers
worked out by hand from the reference's formulas, the category registry, argument checks that fire before any device call."""
import numpy as np
import pytest


@pytest.mark.parametrize("hw, width", [((1080, 1920), 455), ((1080, 2304), 546), ((2160, 3840), 455), ((1920, 1080), 144),
                                       ((200, 300), 384), ((512, 3), 2), ((512, 5), 2)])
def test_keep_ar_width(hw, width):
    from animal_vision_amd.gallery_grid import keep_ar_size

    # new_w = max(1, int(round(w * 256 / h))): 455.1, 546.1, 455.1, 144.0, 384.0, 1.5 -> 2 and 2.5 -> 2 (half to even)
    assert keep_ar_size(*hw, 256) == (256, width)


def test_keep_ar_leaves_a_tile_of_the_target_height_alone():
    from animal_vision_amd.gallery_grid import keep_ar_size

    assert keep_ar_size(256, 999, 256) == (256, 999)
    assert keep_ar_size(1, 1, 256) == (256, 256)
    assert keep_ar_size(4000, 1, 256) == (256, 1)  # max(1, round(0.064))


@pytest.mark.parametrize("n, cols, rows", [(1, 1, 1), (5, 3, 2), (11, 4, 3), (16, 4, 4), (20, 5, 4), (36, 6, 6)])
def test_grid_shape(n, cols, rows):
    from animal_vision_amd.gallery_grid import grid_shape

    assert grid_shape(n) == (cols, rows)


def test_twenty_1080p_tiles_make_the_reference_canvas():
    from animal_vision_amd.gallery_grid import GridLayout

    lay = GridLayout(["Cat"] * 20, [(1080, 1920)] * 20, 256, 8)
    # cell = (256 + 40 + 8) x (455 + 8); 4 rows x 5 cols; canvas = 4 * 304 + 8 by 5 * 463 + 8
    assert (lay.cell_h, lay.cell_w, lay.cols, lay.rows) == (304, 463, 5, 4)
    assert lay.canvas_shape == (1224, 2323, 3)
    assert lay.tile_origin(0) == (8, 8) and lay.tile_origin(6) == (8 + 304, 8 + 463) and lay.tile_origin(19) == (8 + 3 * 304, 8 + 4 * 463)


def test_mixed_tiles_pad_to_the_largest():
    from animal_vision_amd.gallery_grid import GridLayout

    lay = GridLayout(["a", "b", "c"], [(1080, 1920), (1080, 2400), (200, 300)], 256, 13)
    assert lay.sizes == [(256, 455), (256, 569), (256, 384)]
    assert (lay.cell_h, lay.cell_w, lay.cols, lay.rows) == (256 + 40 + 13, 569 + 13, 2, 2)
    assert lay.canvas_shape == (2 * 309 + 13, 2 * 582 + 13, 3)


def test_label_origin():
    from animal_vision_amd.gallery_grid import label_origin
    from animal_vision_amd.renderers.labels import get_text_size

    # "Dog": advances D21 o19 g19 = 59 -> tw = round(59 * 0.6 + 1) = 36, th = round(21 * 0.6 + 1) = 14:
    # x = (455 - 36) // 2 = 209, y = h + 20 + 7 - 2 = h + 25
    assert get_text_size("Dog", 0.6, 1)[0] == (36, 14)
    assert label_origin("Dog", 256, 455) == (209, 256 + 25)
    name = "Anableps (Four-eyed fish)"
    assert get_text_size(name, 0.6, 1)[0][0] == 252
    assert label_origin(name, 256, 455) == (101, 281)  # (455 - 252) // 2
    assert label_origin(name, 256, 144) == (6, 281)    # max(6, negative): the label runs past the tile and is clipped there


def test_segments_are_concatenated_per_tile():
    from animal_vision_amd.gallery_grid import GridLayout
    from animal_vision_amd.renderers.labels import text_segments

    lay = GridLayout(["Dog", "", "Cat"], [(256, 455)] * 3, 256, 8)
    dog, cat = text_segments("Dog", lay.origins[0], 0.6), text_segments("Cat", lay.origins[2], 0.6)
    assert lay.seg_counts == [len(dog), 0, len(cat)] and lay.seg_offsets == [0, len(dog), len(dog)]
    assert lay.segments.dtype == np.float32 and np.array_equal(lay.segments, np.concatenate([dog, cat]))


NON_UV = ["Cat", "Dog", "Sheep", "Pig", "Goat", "Cow", "Horse", "Rabbit", "Panda", "Squirrel", "Elephant", "Lion", "Wolf", "Fox", "Bear",
          "Raccoon", "Deer", "Kangaroo", "Tiger", "Rat"]
UV = ["HoneyBee", "ReinDeer", "RatUV", "GoldFish", "DamselFish", "Anableps (Four-eyed fish)", "Northern Anchovy Fish", "Guppy Fish",
      "Morpho Butterfly", "Heliconius Butterfly", "Pieris Butterfly"]
UNIQUE = ["Mantis Shrimp", "Kestrel", "Jumping Spider", "DragonFly", "HummingBird"]


def test_category_lists_are_the_reference_literals():
    from animal_vision_amd import gallery as G

    assert G.NON_UV_NAMES == NON_UV
    # main.py's UV_NAMES lists the eleven UV species and then, under "# Unique UV animals", the five unique-UV ones
    assert G.UV_NAMES == UV + UNIQUE
    assert G.UNIQUE_UV_NAMES == UNIQUE
    assert G.names_for_category("Non-UV") == NON_UV and G.names_for_category("UV") == UV + UNIQUE and G.names_for_category("Unique-UV") == UNIQUE
    for bad in ("non-uv", "UniqueUV", "", None, "All"):
        with pytest.raises(ValueError):
            G.names_for_category(bad)


def test_registry_maps_every_name_to_its_class():
    from animal_vision_amd import animals as A
    from animal_vision_amd import gallery as G

    want = [A.Cat, A.Dog, A.Sheep, A.Pig, A.Goat, A.Cow, A.Horse, A.Rabbit, A.Panda, A.Squirrel, A.Elephant, A.Lion, A.Wolf, A.Fox, A.Bear,
            A.Raccoon, A.Deer, A.Kangaroo, A.Tiger, A.Rat, A.HoneyBee, A.Reindeer, A.RatUV, A.Goldfish, A.Damselfish, A.Anableps, A.Anchovy,
            A.Guppy, A.Morpho, A.Heliconius, A.Pieris, A.MantisShrimp, A.Kestrel, A.JumpingSpider, A.Dragonfly, A.Hummingbird]
    names = NON_UV + UV + UNIQUE
    assert len(set(names)) == 36
    assert [G.species_class(n) for n in names] == want


def test_gallery_rejects_a_bad_category_before_running_anything():
    from animal_vision_amd import gallery as G

    class Boom:
        def visualize(self, img):
            raise AssertionError("must not run")

    with pytest.raises(ValueError):
        G.gallery(np.zeros((8, 8, 3), np.uint8), "Birds", choices=[("x", Boom())])


def test_ensure_rgb_uint8():
    from animal_vision_amd.gallery import ensure_rgb_uint8

    u = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    assert ensure_rgb_uint8(u) is u
    f = np.array([[[-0.5, 0.0, 0.5], [0.998, 1.0, 7.0]]], np.float32)
    assert ensure_rgb_uint8(f).tolist() == [[[0, 0, 128], [254, 255, 255]]]  # 0.5 * 255 + 0.5 = 128.0; 0.998 * 255 + 0.5 = 254.99
    with pytest.raises(NotImplementedError):
        ensure_rgb_uint8(u.astype(np.int32))


def test_output_name():
    from datetime import datetime

    from animal_vision_amd.gallery import output_name

    t = datetime(2024, 3, 5, 7, 8, 9)
    assert output_name("Non-UV", t) == "gallery_NonUV_20240305_070809.png"
    assert output_name("UV", t) == "gallery_UV_20240305_070809.png"
    assert output_name("Unique-UV", t) == "gallery_UniqueUV_20240305_070809.png"


def test_empty_and_all_none_give_none():
    from animal_vision_amd.gallery_grid import build_labeled_grid

    assert build_labeled_grid([]) is None
    assert build_labeled_grid([("a", None), ("b", None)]) is None


@pytest.mark.parametrize("tiles, kw, exc", [
    ([("a", np.zeros((4, 4), np.uint8))], {}, ValueError),
    ([("a", np.zeros((4, 4, 4), np.uint8))], {}, ValueError),
    ([("a", np.zeros((0, 4, 3), np.uint8))], {}, ValueError),
    ([("a", np.zeros((4, 4, 3), np.float64))], {}, NotImplementedError),
    ([("a", np.zeros((4, 4, 3), np.uint16))], {}, NotImplementedError),
    ([("a", [[1, 2, 3]])], {}, ValueError),
    ([(3, np.zeros((4, 4, 3), np.uint8))], {}, TypeError),
    ([np.zeros((4, 4, 3), np.uint8)], {}, ValueError),
    ([("a", np.zeros((4, 4, 3), np.uint8))], {"tile_height": 0}, ValueError),
    ([("a", np.zeros((4, 4, 3), np.uint8))], {"tile_height": 2.5}, ValueError),
    ([("a", np.zeros((4, 4, 3), np.uint8))], {"pad": -1}, ValueError),
    ([("a", np.zeros((4, 4, 3), np.uint8))], {"bg": (0, 0)}, ValueError),
    ([("a", np.zeros((4, 4, 3), np.uint8))], {"bg": (0, 0, 256)}, ValueError),
    ([("a", np.zeros((4, 4, 3), np.uint8))], {"bg": (0, -1, 0)}, ValueError),
])
def test_malformed_arguments_raise_before_the_device(tiles, kw, exc, monkeypatch):
    from animal_vision_amd import runtime
    from animal_vision_amd.gallery_grid import build_labeled_grid

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(runtime, "get_context", no_device)
    with pytest.raises(exc):
        build_labeled_grid(tiles, **kw)
