"""The column walk of the marching FeedForward kernel (csrc/mst_tile_order.h, ColumnWalk), run on the host through avx_mst_tile_order_col: every tile of a
(frames x ty x tx) grid is visited exactly once whatever the workgroup count; a workgroup's tiles are consecutive positions of the column-major order (frame,
tile column, tile row) -- consecutive rows of one column, except where the next column begins; and a segment start is flagged at every workgroup's first tile
and at the top of every column, nowhere else (there the kernel computes the two top halo rows, everywhere else it carries them from the tile above)."""
import ctypes

import numpy as np
import pytest


def _walk(frames, ty, tx, nwg):
    from animal_vision_amd._lib import lib

    steps = ctypes.c_int(0)
    assert lib.avx_mst_tile_order_col(frames, ty, tx, nwg, None, None, 0, ctypes.byref(steps)) == 0
    v = np.empty((nwg, max(steps.value, 1)), np.int64)
    seg = np.full(v.shape, 7, np.uint8)
    assert lib.avx_mst_tile_order_col(frames, ty, tx, nwg, v.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), seg.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                      v.shape[1], ctypes.byref(steps)) == 0
    return v, seg


def _check(frames, ty, tx, nwg):
    what = (frames, ty, tx, nwg)
    total = frames * ty * tx
    v, seg = _walk(frames, ty, tx, nwg)
    live = v >= 0
    assert np.array_equal(np.sort(v[live]), np.arange(total)), what  # every tile exactly once
    assert (live[:, :-1] >= live[:, 1:]).all(), what  # a workgroup's steps have no holes
    n = live.sum(1)
    assert n.min() >= total // nwg and n.max() <= -(-total // nwg), what  # balanced to one tile
    vv = np.maximum(v, 0)
    b, y, x = vv // (ty * tx), (vv // tx) % ty, vv % tx
    pos = (b * tx + x) * ty + y  # column-major: frame, tile column, tile row
    k = np.arange(v.shape[1])[None, :]
    assert np.array_equal(np.where(live, pos, -1), np.where(live, pos[:, :1] + k, -1)), what  # one contiguous run each
    # so a step goes to the next row of the same column, or from a column's last row to the top of the next column (of the next frame behind the last column)
    same_col = live[:, 1:] & (x[:, 1:] == x[:, :-1]) & (b[:, 1:] == b[:, :-1])
    assert (y[:, 1:][same_col] == y[:, :-1][same_col] + 1).all(), what
    turn = live[:, 1:] & ~same_col
    assert (y[:, 1:][turn] == 0).all() and (y[:, :-1][turn] == ty - 1).all(), what
    # segment starts: a workgroup's first tile, every column top, nothing else; nothing past the walk's end
    assert np.array_equal(seg, (live & ((k == 0) | (y == 0))).astype(np.uint8)), what
    # the workgroups of a class (index % 8) own neighbouring runs, the classes' stretches in order
    lo = 0
    for g in range(min(8, nwg)):
        first, cnt = pos[g::8, 0], n[g::8]
        for f, c in zip(first, cnt):
            if c:
                assert f == lo, (what, g)
                lo += c
    assert lo == total, what


@pytest.mark.parametrize("frames", [1, 2, 3])
def test_column_walk_visits_every_tile_once_in_runs_and_flags_segment_starts(frames):
    """ty, tx over 1 ... 40 in full; per grid three workgroup counts drawn from 1 ... 512 (seeded), and more workgroups than tiles for every seventh grid."""
    rng = np.random.default_rng(100 + frames)
    for ty in range(1, 41):
        for tx in range(1, 41):
            nwgs = [int(n) for n in rng.integers(1, 513, 3)]
            if (ty + tx) % 7 == 0:
                nwgs.append(frames * ty * tx + 5)
            for nwg in nwgs:
                _check(frames, ty, tx, nwg)


@pytest.mark.parametrize("grid", [(1, 1, 1), (1, 3, 5), (2, 7, 4), (3, 40, 40), (1, 155, 240)])
def test_column_walk_at_every_workgroup_count(grid):
    """workgroups 1 ... 512 in full (and more than tiles) on a few grids; (1, 155, 240) is a 4K frame in 16 x 14 tiles"""
    frames, ty, tx = grid
    for nwg in list(range(1, 513)) + [frames * ty * tx + 5]:
        _check(frames, ty, tx, nwg)


def test_column_walk_refuses_empty_grids():
    from animal_vision_amd._lib import lib

    steps = ctypes.c_int(0)
    for args in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert lib.avx_mst_tile_order_col(*args, None, None, 0, ctypes.byref(steps)) != 0
