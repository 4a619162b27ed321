"""The steps of the marching attention tail (csrc/mst_tile_order.h, ColumnSteps), run on the host through avx_mst_tail_march_steps: they are the column walk of
avx_mst_tile_order_col with one priming step put in front of every tile that starts a segment, and nowhere else -- the step the kernel runs on the tile above
(stores masked) to get on chip what it carries from tile to tile everywhere else."""
import ctypes

import numpy as np
import pytest

_LL, _UB = ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ubyte)


def _steps(frames, ty, tx, nwg):
    from animal_vision_amd._lib import lib

    n = ctypes.c_int(0)
    assert lib.avx_mst_tail_march_steps(frames, ty, tx, nwg, None, None, 0, ctypes.byref(n)) == 0
    v = np.empty((nwg, max(n.value, 1)), np.int64)
    prime = np.full(v.shape, 7, np.uint8)
    assert lib.avx_mst_tail_march_steps(frames, ty, tx, nwg, v.ctypes.data_as(_LL), prime.ctypes.data_as(_UB), v.shape[1], ctypes.byref(n)) == 0
    return v, prime, n.value


def _walk(frames, ty, tx, nwg):
    from animal_vision_amd._lib import lib

    n = ctypes.c_int(0)
    assert lib.avx_mst_tile_order_col(frames, ty, tx, nwg, None, None, 0, ctypes.byref(n)) == 0
    v = np.empty((nwg, max(n.value, 1)), np.int64)
    seg = np.empty(v.shape, np.uint8)
    assert lib.avx_mst_tile_order_col(frames, ty, tx, nwg, v.ctypes.data_as(_LL), seg.ctypes.data_as(_UB), v.shape[1], ctypes.byref(n)) == 0
    return v, seg


def _check(frames, ty, tx, nwg):
    what = (frames, ty, tx, nwg)
    v, prime, most = _steps(frames, ty, tx, nwg)
    wv, seg = _walk(frames, ty, tx, nwg)
    assert set(np.unique(prime)) <= {0, 1}, what
    longest = 0
    for wg in range(nwg):
        tiles, segs = wv[wg][wv[wg] >= 0], seg[wg][wv[wg] >= 0]
        want_v, want_p = [], []
        for t, s in zip(tiles, segs):  # the walk, a priming step in front of each segment start
            if s:
                want_v.append(t)
                want_p.append(1)
            want_v.append(t)
            want_p.append(0)
        n = len(want_v)
        longest = max(longest, n)
        assert v[wg, :n].tolist() == want_v and prime[wg, :n].tolist() == want_p, (what, wg)
        assert (v[wg, n:] == -1).all() and (prime[wg, n:] == 0).all(), (what, wg)  # nothing past the walk's end
    assert most == longest, what
    real = v[(v >= 0) & (prime == 0)]
    assert np.array_equal(np.sort(real), np.arange(frames * ty * tx)), what  # every tile computed exactly once


@pytest.mark.parametrize("grid", [(1, 1, 1), (1, 1, 7), (1, 5, 1), (2, 5, 3), (3, 2, 2), (1, 270, 138), (1, 78, 138)])
def test_march_steps_put_one_priming_step_in_front_of_every_segment(grid):
    """(1, 270, 138): a 4K frame in 28 x 8 tiles; (1, 78, 138): 1080 x 1920 in 14 x 14 tiles"""
    frames, ty, tx = grid
    total = frames * ty * tx
    for nwg in sorted({1, 2, 3, 5, 8, 9, 64, 255, 256, 512} | ({total, total + 5} if total < 1000 else set())):
        _check(frames, ty, tx, nwg)


def test_march_steps_refuse_empty_grids():
    from animal_vision_amd._lib import lib

    n = ctypes.c_int(0)
    for args in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert lib.avx_mst_tail_march_steps(*args, None, None, 0, ctypes.byref(n)) != 0
