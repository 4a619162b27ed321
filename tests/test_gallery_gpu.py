"""GPU: the species gallery (csrc/gallery.hip avx_gallery_compose_u8; reference: gallery_grid.py:8-106, main.py:203-278).

The montage is pinned twice: against the oracle's restatement of build_labeled_grid below (oracle.cv_resize INTER_AREA,
_to_uint8, a black strip, oracle.draw_label_pixels with the strip as its box, NumPy padding and placement) and against the
same canvas put together from the existing entry points (avx_resize_hwc, avx_draw_label_u8, one call per tile)."""
import ctypes
import re
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NON_UV = ["Cat", "Dog", "Sheep", "Pig", "Goat", "Cow", "Horse", "Rabbit", "Panda", "Squirrel", "Elephant", "Lion", "Wolf", "Fox", "Bear",
          "Raccoon", "Deer", "Kangaroo", "Tiger", "Rat"]
LONGEST = "Anableps (Four-eyed fish)"


def _keep_ar(h, w, tile_height):
    return (h, w) if h == tile_height else (tile_height, max(1, int(round(w * (tile_height / float(h))))))


def _place(tiles, pad, bg):
    """build_labeled_grid's steps 5-6 on finished tile-plus-strip images."""
    max_h, max_w = max(t.shape[0] for t in tiles), max(t.shape[1] for t in tiles)
    n = len(tiles)
    cols = int(np.ceil(np.sqrt(n)))
    rows = -(-n // cols)
    cell_h, cell_w = max_h + pad, max_w + pad
    grid = np.empty((rows * cell_h + pad, cols * cell_w + pad, 3), np.uint8)
    grid[...] = np.asarray(bg, np.uint8)
    for i, t in enumerate(tiles):
        r, c = divmod(i, cols)
        y, x = pad + r * cell_h, pad + c * cell_w
        grid[y : y + t.shape[0], x : x + t.shape[1]] = t
    return grid


def _to_uint8(img):
    return img if img.dtype == np.uint8 else (np.clip(img, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def _label_args(name, h, w):
    from animal_vision_amd.renderers.labels import get_text_size, text_segments

    (tw, th), _ = get_text_size(name, 0.6, 1)
    org = (max(6, (w - tw) // 2), h + 40 // 2 + th // 2 - 2)
    return (0, h, w - 1, h + 39), text_segments(name, org, 0.6)


def oracle_grid(tiles, tile_height=256, pad=8, bg=(20, 20, 20)):
    """build_labeled_grid restated on the oracle."""
    from oracle import cpu_ref

    out = []
    for name, img in tiles:
        if img is None:
            continue
        h, w = _keep_ar(*img.shape[:2], tile_height)
        if (h, w) != img.shape[:2]:
            img = cpu_ref.cv_resize(img, (w, h), cpu_ref.INTER_AREA)
        img = _to_uint8(img)
        t = np.vstack([img, np.zeros((40, w, 3), np.uint8)])
        box, segs = _label_args(name, h, w)
        cpu_ref.draw_label_pixels(t, box, segs, 3, 1)
        out.append(t)
    return _place(out, pad, bg) if out else None


def entry_point_grid(tiles, tile_height=256, pad=8, bg=(20, 20, 20)):
    """The same canvas from the existing entry points: avx_resize_hwc and avx_draw_label_u8 per tile, placed with NumPy."""
    from animal_vision_amd._lib import lib
    from animal_vision_amd.geometry import INTER_AREA, resize_device
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    out = []
    for name, img in tiles:
        h, w = _keep_ar(*img.shape[:2], tile_height)
        if (h, w) != img.shape[:2]:
            d = ctx.upload(np.ascontiguousarray(img))
            r = resize_device(ctx, d, img.dtype, img.shape[0], img.shape[1], 3, h, w, INTER_AREA)
            img = ctx.download(r, (h, w, 3), img.dtype)
            d.free()
            r.free()
        t = np.vstack([_to_uint8(img), np.zeros((40, w, 3), np.uint8)])
        box, segs = _label_args(name, h, w)
        d = ctx.upload(t)
        segs = np.ascontiguousarray(segs)
        ctx._check(lib.avx_draw_label_u8(ctx._h, d.ptr, h + 40, w, (ctypes.c_int * 4)(*box), segs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                         len(segs), 3.0, 1.0, 0, ctx._s(None)))
        out.append(ctx.download(d, t.shape, np.uint8))
        d.free()
    return _place(out, pad, bg)


def _frames(shapes, seed=0):
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    return [(noise_frame if i % 2 else structured_frame)(seed + i, h, w) for i, (h, w) in enumerate(shapes)]


def _check(tiles, **kw):
    from animal_vision_amd.gallery_grid import build_labeled_grid

    got = build_labeled_grid(tiles, **kw)
    want = oracle_grid(tiles, **kw)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, f"{len(bad)} pixels differ from the oracle, first at {bad[:3].tolist()}"
    return got


def test_twenty_1080p_tiles_equal_the_oracle():
    tiles = list(zip(NON_UV, _frames([(1080, 1920)] * 20)))
    got = _check(tiles)
    assert got.shape == (1224, 2323, 3)


def test_mixed_widths_equal_the_oracle():
    _check(list(zip(["Dog", "Northern Anchovy Fish", "Morpho Butterfly", "Cat"], _frames([(1080, 1920), (1080, 2304), (1080, 2400), (720, 1280)], 3))))


def test_special_sizes_equal_the_oracle():
    """No resize (already 256 high), enlarging (INTER_LINEAR), integer ratios 4 and 2 (the 8-bit 2x2 rounding), an odd size,
    and a portrait tile whose label is wider than the tile (clipped at its right edge)."""
    shapes = [(256, 300), (200, 300), (1024, 1536), (512, 768), (97, 131), (1920, 1080)]
    names = ["Kestrel", "Pig", "RatUV", "Guppy Fish", "Fox", LONGEST]
    got = _check(list(zip(names, _frames(shapes, 7))))
    # the portrait tile is 144 wide: the text stops at its edge, the padding to its right is bg
    assert got.shape[1] == 3 * (384 + 8) + 8


@pytest.mark.parametrize("tile_height, pad, bg", [(128, 0, (0, 0, 0)), (300, 13, (255, 128, 7)), (256, 8, (20, 20, 20))])
def test_layout_parameters_equal_the_oracle(tile_height, pad, bg):
    shapes = [(1080, 1920), (300, 300), (97, 131), (720, 1280), (1920, 1080)]
    _check(list(zip(["Cat", "ReinDeer", "Fox", "Mantis Shrimp", LONGEST], _frames(shapes, 11))), tile_height=tile_height, pad=pad, bg=bg)


def test_float_tiles_equal_the_oracle():
    rng = np.random.default_rng(5)
    shapes = [(1080, 1920), (256, 200), (200, 300), (1024, 1536), (97, 131)]
    tiles = [(f"f{i}", rng.uniform(-0.3, 1.3, (h, w, 3)).astype(np.float32)) for i, (h, w) in enumerate(shapes)]
    tiles.append(("mixed", _frames([(540, 960)])[0]))
    _check(tiles)


def test_none_tiles_are_dropped():
    frames = _frames([(300, 400), (300, 400)])
    from animal_vision_amd.gallery_grid import build_labeled_grid

    assert np.array_equal(build_labeled_grid([("a", frames[0]), ("b", None), ("c", frames[1])]), oracle_grid([("a", frames[0]), ("c", frames[1])]))


@pytest.mark.parametrize("which", ["1080p", "mixed"])
def test_montage_equals_the_existing_entry_points(which):
    from animal_vision_amd.gallery_grid import build_labeled_grid

    if which == "1080p":
        tiles = list(zip(NON_UV[:6], _frames([(1080, 1920)] * 6, 20)))
    else:
        shapes = [(256, 300), (200, 300), (1024, 1536), (512, 768), (97, 131), (1920, 1080)]
        tiles = list(zip(["Kestrel", "Pig", "RatUV", "Guppy Fish", "Fox", LONGEST], _frames(shapes, 30)))
        tiles.append(("float", np.random.default_rng(1).uniform(-0.2, 1.2, (400, 500, 3)).astype(np.float32)))
    assert np.array_equal(build_labeled_grid(tiles), entry_point_grid(tiles))


class _Recorder:
    """A registry species that remembers what visualize returned."""

    seen = {}

    def __init__(self, name, cls):
        self.name, self.sp = name, cls()

    def visualize(self, img):
        res = self.sp.visualize(img)
        _Recorder.seen[self.name] = res
        return res


@pytest.mark.parametrize("category, hw", [("Non-UV", (1080, 1920)), ("UV", (1080, 1920)), ("Unique-UV", (1080, 1920)), ("Unique-UV", (2160, 3840))])
def test_gallery_equals_the_grid_of_the_species_outputs(monkeypatch, category, hw):
    from animal_vision_amd import gallery as G
    from animal_vision_amd.gallery_grid import build_labeled_grid
    from animal_vision_amd.synthetic import structured_frame

    real = G.species_class
    monkeypatch.setattr(G, "species_class", lambda name: (lambda: _Recorder(name, real(name))))
    _Recorder.seen = {}
    frame = structured_frame(0, *hw)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = G.gallery(frame, category)
    assert not [w for w in caught if str(w.message).startswith("gallery:")], "every registry species runs"
    names = G.names_for_category(category)
    assert list(_Recorder.seen) == names
    tiles = []
    for n in names:
        base, out = _Recorder.seen[n]
        tiles.append((n, out if out is not None else base))
    assert np.array_equal(got, build_labeled_grid(tiles))


def test_failing_species_are_skipped_with_a_warning():
    from animal_vision_amd.gallery import gallery
    from animal_vision_amd.gallery_grid import build_labeled_grid

    frame = _frames([(120, 160)])[0]

    class Boom:
        def visualize(self, img):
            raise RuntimeError("no such band")

    class BaseOnly:
        def visualize(self, img):
            return img[::-1].copy(), None

    class Float:
        def visualize(self, img):
            return img, img.astype(np.float32) / 200.0  # values above 1: clipped by _ensure_rgb_uint8

    with pytest.warns(RuntimeWarning, match=r"Boom species.*RuntimeError.*no such band"):
        got = gallery(frame, "UV", choices=[("Boom species", Boom()), ("base", BaseOnly()), ("float", Float())])
    f = frame.astype(np.float32) / 200.0
    want = build_labeled_grid([("base", frame[::-1].copy()), ("float", (np.clip(f, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8))])
    assert np.array_equal(got, want)
    with pytest.warns(RuntimeWarning):
        assert gallery(frame, "Non-UV", choices=[("x", Boom())]) is None


def test_main_writes_the_reference_file_name(tmp_path, capsys):
    from PIL import Image

    from animal_vision_amd.gallery import gallery, main

    frame = _frames([(96, 128)])[0]
    src = tmp_path / "in.png"
    Image.fromarray(frame).save(src)
    out_dir = tmp_path / "out"
    assert main([str(src), "--category", "Non-UV", "--tile-height", "64", "--output-dir", str(out_dir)]) == 0
    files = list(out_dir.iterdir())
    assert len(files) == 1 and re.fullmatch(r"gallery_NonUV_\d{8}_\d{6}\.png", files[0].name)
    assert str(files[0]) in capsys.readouterr().out
    assert np.array_equal(np.asarray(Image.open(files[0]).convert("RGB")), gallery(frame, "Non-UV", tile_height=64))


def test_invalid_descriptors_fail_and_the_context_stays_usable():
    from animal_vision_amd._lib import AVX_ERR_INVALID, AvxError, GalleryTile, lib
    from animal_vision_amd.gallery_grid import build_labeled_grid
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    src = ctx.upload(np.zeros((64, 64, 3), np.uint8))
    canvas = ctx.malloc(200 * 200 * 3)
    segs = np.zeros((4, 6), np.float32)
    fp = segs.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    bg = (ctypes.c_int * 3)(20, 20, 20)

    def call(tile=None, n=1, nseg=4, cols=1, Hc=200, Wc=200, bgv=bg, strip=40, pad=8):
        t = tile or GalleryTile(src.ptr, 2, 64, 64, 32, 32, 0, 4)
        arr = (GalleryTile * 1)(t)
        return lib.avx_gallery_compose_u8(ctx._h, arr, n, fp, nseg, strip, pad, cols, bgv, canvas.ptr, Hc, Wc, ctx._s(None))

    assert call() == 0
    bad = [
        dict(n=0),
        dict(tile=GalleryTile(src.ptr, 1, 64, 64, 32, 32, 0, 4)),        # dtype 1
        dict(tile=GalleryTile(src.ptr, 2, 64, 64, 32, 32, 2, 4)),        # segments [2, 6) of 4
        dict(tile=GalleryTile(src.ptr, 2, 64, 64, 32, 32, -1, 1)),
        dict(tile=GalleryTile(None, 2, 64, 64, 32, 32, 0, 4)),
        dict(tile=GalleryTile(src.ptr, 2, 0, 64, 32, 32, 0, 4)),
        dict(tile=GalleryTile(src.ptr, 2, 64, 64, 190, 32, 0, 4)),       # 190 + 40 + 16 rows > 200: outside the canvas
        dict(Wc=40),                                                    # 32 + 16 > 40
        dict(cols=0), dict(pad=-1), dict(strip=-1), dict(nseg=-1), dict(Hc=0),
        dict(bgv=(ctypes.c_int * 3)(0, 256, 0)),
    ]
    for kw in bad:
        rc = call(**kw)
        assert rc == AVX_ERR_INVALID, kw
        with pytest.raises(AvxError, match="avx_gallery_compose_u8"):
            ctx._check(rc)
    ctx.sync()
    src.free()
    canvas.free()
    frames = _frames([(80, 100)])
    assert np.array_equal(build_labeled_grid([("ok", frames[0])], tile_height=40), oracle_grid([("ok", frames[0])], tile_height=40))
