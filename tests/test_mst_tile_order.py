"""The tile order of the persistent MST++ tile kernels (csrc/mst_tile_order.h), run on the host through avx_mst_tile_order: every tile of a
(frames x ty x tx) grid is visited exactly once whatever the workgroup count, and the workgroups that share an XCD (index % 8) walk one
contiguous stretch of the band-major order together."""
import ctypes

import numpy as np
import pytest

SIDES = (1, 3, 135, 240, 275)      # 4K: 135 tile rows of 16, 240 (16 px) or 275 (14 px) tile columns
NWGS = (1, 7, 8, 9, 256, 257, 512)  # fewer than 8, ragged against 8, the launch sizes of a 256-CU part


def _visit(frames, ty, tx, nwg, raster):
    from animal_vision_amd._lib import lib

    steps = ctypes.c_int(0)
    assert lib.avx_mst_tile_order(frames, ty, tx, nwg, raster, None, 0, ctypes.byref(steps)) == 0
    v = np.empty((nwg, max(steps.value, 1)), np.int64)
    assert lib.avx_mst_tile_order(frames, ty, tx, nwg, raster, v.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), v.shape[1], ctypes.byref(steps)) == 0
    return v


def _band_major(frames, ty, tx):
    """position of every tile (by raster index) in the band-major order: min(8, tx) bands of tile columns, the first tx % nb one column wider,
    each walked frame by frame and row by row; and the band of every tile"""
    nb = min(8, tx)
    qb, rb = divmod(tx, nb)
    widths = np.array([qb + 1] * rb + [qb] * (nb - rb))
    x0 = np.concatenate([[0], np.cumsum(widths)[:-1]])
    band_of_col = np.repeat(np.arange(nb), widths)
    b, y, x = np.meshgrid(np.arange(frames), np.arange(ty), np.arange(tx), indexing="ij")
    band = band_of_col[x]
    pos = x0[band] * ty * frames + (b * ty + y) * widths[band] + (x - x0[band])
    return pos.reshape(-1), band.reshape(-1)


@pytest.mark.parametrize("tx", SIDES)
@pytest.mark.parametrize("ty", SIDES)
def test_tile_order_visits_every_tile_once_and_keeps_an_xcd_on_one_stretch(ty, tx):
    for frames in (1, 2, 3, 4):
        total = frames * ty * tx
        pos, _ = _band_major(frames, ty, tx)
        assert np.array_equal(np.sort(pos), np.arange(total))  # the test's own order is a permutation
        for nwg in NWGS + (total + 5,):  # and more workgroups than tiles
            v = _visit(frames, ty, tx, nwg, 0)
            live = v >= 0
            assert np.array_equal(np.sort(v[live]), np.arange(total)), (frames, ty, tx, nwg)
            assert (live[:, :-1] >= live[:, 1:]).all()  # a workgroup's steps have no holes
            # balanced: nobody takes more than one tile above the even share
            assert live.sum(1).max() <= -(-total // nwg) + 1, (frames, ty, tx, nwg, live.sum(1).max())
            lo_prev = 0
            for g in range(min(8, nwg)):
                vg = v[g::8]
                n = vg.shape[0]
                pg = np.where(vg >= 0, pos[np.maximum(vg, 0)], -1)
                mine = np.sort(pg[pg >= 0])
                if mine.size == 0:
                    continue
                # one contiguous stretch of the band-major order, the classes' stretches in order
                assert mine[0] == lo_prev and np.array_equal(mine, np.arange(mine[0], mine[0] + mine.size)), (frames, ty, tx, nwg, g)
                lo_prev = mine[-1] + 1
                # and at every step the tiles in flight are consecutive positions: member m is at first + step * n + m
                want = mine[0] + n * np.arange(pg.shape[1])[None, :] + np.arange(n)[:, None]
                assert np.array_equal(pg, np.where(want <= mine[-1], want, -1)), (frames, ty, tx, nwg, g)
            assert lo_prev == total
            # the raster switch: tiles wg, wg + nwg, ...
            r = _visit(frames, ty, tx, nwg, 1)
            want = np.arange(nwg)[:, None] + nwg * np.arange(r.shape[1])[None, :]
            assert np.array_equal(r, np.where(want < total, want, -1)), (frames, ty, tx, nwg)


@pytest.mark.parametrize("nwg", [8, 256, 512])
@pytest.mark.parametrize("frames", [1, 2])
def test_an_xcd_owns_a_band_of_tile_columns_where_the_grid_divides_by_eight(frames, nwg):
    """tx = 240 (4K in 16-pixel columns), workgroup counts that are multiples of 8: class g's stretch IS band g, columns 30 g ... 30 g + 29 of every row of every frame."""
    ty, tx = 135, 240
    v = _visit(frames, ty, tx, nwg, 0)
    for g in range(8):
        vg = v[g::8]
        cols = np.unique(vg[vg >= 0] % tx)
        assert np.array_equal(cols, np.arange(30 * g, 30 * g + 30))
        assert (vg >= 0).sum() == frames * ty * 30


def test_ragged_grid_laps_only_a_little_into_the_neighbouring_band():
    """tx = 275 (4K in 14-pixel columns): bands are 35 or 34 columns wide, the classes' shares are equal, so a class's stretch starts a little inside its neighbour's band:
    by at most the three extra columns of the wide bands (3 x 135 tiles of its 4,640), so at least 90 % of its tiles lie in ONE band."""
    frames, ty, tx, nwg = 1, 135, 275, 512
    v = _visit(frames, ty, tx, nwg, 0)
    _, band = _band_major(frames, ty, tx)
    for g in range(8):
        vg = v[g::8]
        counts = np.bincount(band[vg[vg >= 0]], minlength=8)
        assert counts.max() >= 0.9 * counts.sum() and np.count_nonzero(counts) <= 2, (g, counts)


def test_tile_order_refuses_empty_grids():
    from animal_vision_amd._lib import lib

    steps = ctypes.c_int(0)
    for args in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert lib.avx_mst_tile_order(*args, 0, None, 0, ctypes.byref(steps)) != 0
