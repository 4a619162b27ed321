"""gallery_grid.build_labeled_grid (reference: gallery_grid.py:8-106): the labelled contact sheet of the `gallery` command.

The host restates the reference's layout -- keep-aspect tile sizes (_resize_keep_ar), the label origin (_label_strip), the
padded cells and the row-major grid -- and csrc/gallery.hip composes the whole canvas in one launch: every tile resized with
avx_resize_hwc's INTER_AREA arithmetic, converted as _to_uint8 converts it, its 40-row black strip, its Hershey-simplex label
drawn as avx_draw_label_u8 draws it (clipped to the tile), the bg padding.  The layout helpers below touch no device."""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .renderers.labels import get_text_size, text_segments

STRIP_H = 40           # _label_strip's strip height
LABEL_SCALE = 0.6      # cv2.putText(FONT_HERSHEY_SIMPLEX, 0.6) ...
LABEL_THICKNESS = 1    # ... thickness 1 for the text, + 2 for its outline (fixed in csrc/gallery.hip)
_DTYPES = {np.dtype(np.float32): 0, np.dtype(np.uint8): 2}  # avx_gallery_tile.dtype


def keep_ar_size(h: int, w: int, tile_height: int) -> Tuple[int, int]:
    """_resize_keep_ar: (h, w) unchanged when h == tile_height, else (tile_height, max(1, round(w * tile_height / h))) with
    Python's round (half to even)."""
    if h == tile_height:
        return h, w
    return tile_height, max(1, int(round(w * (tile_height / float(h)))))


def label_origin(text: str, h: int, w: int, strip_h: int = STRIP_H) -> Tuple[int, int]:
    """_label_strip's text origin on the (h + strip_h) x w tile-plus-strip image: centred, at least 6 px from the left."""
    (tw, th), _ = get_text_size(text, LABEL_SCALE, LABEL_THICKNESS)
    return max(6, (w - tw) // 2), h + strip_h // 2 + th // 2 - 2


def grid_shape(n: int) -> Tuple[int, int]:
    """(cols, rows) of n tiles: cols = ceil(sqrt(n)), rows = ceil(n / cols)."""
    cols = math.ceil(math.sqrt(n))
    return cols, math.ceil(n / cols)


class GridLayout:
    """Everything about a sheet except its pixels: per tile the resized size, label origin and segment rows; the grid."""

    def __init__(self, labels: Sequence[str], shapes: Sequence[Tuple[int, int]], tile_height: int, pad: int):
        self.sizes = [keep_ar_size(h, w, tile_height) for h, w in shapes]
        self.origins = [label_origin(t, h, w) for t, (h, w) in zip(labels, self.sizes)]
        segs = [text_segments(t, o, LABEL_SCALE) for t, o in zip(labels, self.origins)]
        self.seg_offsets = np.cumsum([0] + [len(s) for s in segs])[:-1].tolist()
        self.seg_counts = [len(s) for s in segs]
        self.segments = np.ascontiguousarray(np.concatenate(segs, 0) if sum(self.seg_counts) else np.zeros((0, 6), np.float32), np.float32)
        self.cols, self.rows = grid_shape(len(self.sizes))
        self.cell_h = max(h for h, _ in self.sizes) + STRIP_H + pad
        self.cell_w = max(w for _, w in self.sizes) + pad
        self.pad = pad
        self.canvas_shape = (self.rows * self.cell_h + pad, self.cols * self.cell_w + pad, 3)

    def tile_origin(self, i: int) -> Tuple[int, int]:
        """(y, x) of tile i's top-left pixel on the canvas (row-major)."""
        r, c = divmod(i, self.cols)
        return self.pad + r * self.cell_h, self.pad + c * self.cell_w


def check_tiles(tiles, tile_height: int, pad: int, bg) -> List[Tuple[str, np.ndarray]]:
    """Validate the arguments of build_labeled_grid without touching a device; returns the tiles that are not None."""
    if isinstance(tile_height, bool) or not isinstance(tile_height, (int, np.integer)) or tile_height < 1:
        raise ValueError(f"tile_height must be an integer >= 1 (got {tile_height!r})")
    if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or pad < 0:
        raise ValueError(f"pad must be an integer >= 0 (got {pad!r})")
    bgl = list(bg) if isinstance(bg, (tuple, list, np.ndarray)) else None
    if bgl is None or len(bgl) != 3 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 255 for v in bgl):
        raise ValueError(f"bg must be three integers in 0..255 (got {bg!r})")
    kept = []
    for item in tiles:
        if not isinstance(item, (tuple, list)) or len(item) != 2:
            raise ValueError("tiles must be (label, image) pairs")
        label, img = item
        if img is None:
            continue
        if not isinstance(label, str):
            raise TypeError(f"a tile label must be a str (got {type(label).__name__})")
        if not isinstance(img, np.ndarray) or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError(f"tile {label!r}: expected an HxWx3 image (got {getattr(img, 'shape', type(img).__name__)})")
        if img.dtype not in _DTYPES:
            raise NotImplementedError(f"tile {label!r}: dtype {img.dtype} (uint8 and float32 tiles are supported)")
        kept.append((label, img))
    return kept


_arena = {}  # per context: the device buffer the tiles are uploaded into and the canvas buffer, grown on demand


def _buffer(ctx, key: str, nbytes: int):
    buf = _arena.get((id(ctx), key))
    if buf is None or buf.nbytes < nbytes:
        if buf is not None:
            buf.free()
        buf = ctx.malloc(max(nbytes, 1 << 20))
        _arena[(id(ctx), key)] = buf
    return buf


def build_labeled_grid(
    tiles: List[Tuple[str, np.ndarray]],
    *,
    tile_height: int = 256,
    pad: int = 8,
    bg: Tuple[int, int, int] = (20, 20, 20),
) -> Optional[np.ndarray]:
    """tiles: (label, HxWx3 RGB image) pairs, uint8 or float32 in [0, 1]; None images are dropped.  Returns the RGB uint8 grid,
    or None when no tile is left.  One upload per tile into one device arena, one compose launch, one download."""
    from ._lib import GalleryTile, lib
    from .runtime import get_context

    kept = check_tiles(tiles, tile_height, pad, bg)
    if not kept:
        return None
    lay = GridLayout([t for t, _ in kept], [img.shape[:2] for _, img in kept], int(tile_height), int(pad))
    ctx = get_context()
    arrays = [np.ascontiguousarray(img) for _, img in kept]
    offsets, total = [], 0
    for a in arrays:
        offsets.append(total)
        total += (a.nbytes + 255) & ~255
    d_tiles = _buffer(ctx, "tiles", total)
    Hc, Wc, _ = lay.canvas_shape
    d_canvas = _buffer(ctx, "canvas", Hc * Wc * 3)
    desc = (GalleryTile * len(arrays))()
    s = ctx._s(None)
    for i, a in enumerate(arrays):
        ctx._check(lib.avx_memcpy_h2d(ctx._h, d_tiles.ptr + offsets[i], a.ctypes.data, a.nbytes, s))
        h, w = lay.sizes[i]
        desc[i] = GalleryTile(d_tiles.ptr + offsets[i], _DTYPES[a.dtype], a.shape[0], a.shape[1], h, w, lay.seg_offsets[i], lay.seg_counts[i])
    bg_c = (ctypes.c_int * 3)(*(int(v) for v in bg))
    segs = lay.segments
    rc = lib.avx_gallery_compose_u8(ctx._h, desc, len(arrays), segs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(segs), STRIP_H, int(pad),
                                    lay.cols, bg_c, d_canvas.ptr, Hc, Wc, s)
    if rc:
        ctx.sync()  # the uploads read `arrays`: let them finish before the error unwinds
        ctx._check(rc)
    return ctx.download(d_canvas, lay.canvas_shape, np.uint8)  # synchronises: the uploads are done too
