"""The device loop of the pair commands (animal_vision_amd/pairs.py, stream_pairs) without a device: a fake context whose streams
queue their work until they are synchronised, as a device does, and fake sources that hand out numbered 4 x 6 frames.  The "kernel"
is A xor B.  What is pinned: the order and contents of the items, info["longer"], that a buffer set is never filled while its
previous batch is in flight, and that every buffer, stream and source is released exactly once however the generator ends."""
import itertools
import types

import numpy as np
import pytest

from animal_vision_amd import pairs

H, W = 4, 6
UNIT = H * W * 3


def _frame(seed: int, i: int) -> np.ndarray:
    return ((np.arange(UNIT) * 7 + 13 * i + seed) % 256).astype(np.uint8).reshape(H, W, 3)


class _Tracked:
    """A staging array that knows whether work queued on a stream still reads or writes it."""

    def __init__(self, owner, shape):
        self.owner, self.data = owner, np.zeros(shape, np.uint8)

    def __setitem__(self, key, value):
        assert self.owner.stream is None, "a set is filled while its previous batch is in flight"
        self.data[key] = value

    def __getitem__(self, key):
        assert self.owner.stream is None, "staging is read before its stream was synchronised"
        return self.data[key]


class _Buf:
    def __init__(self, shape, pinned):
        self.freed, self.stream = 0, None  # stream: the one with queued work on this buffer
        self.array = _Tracked(self, shape) if pinned else np.zeros(shape, np.uint8)
        self.ptr = id(self)

    def bytes(self):
        return (self.array.data if isinstance(self.array, _Tracked) else self.array).reshape(-1)

    def free(self):
        self.freed += 1


class _Ctx:
    """stream_create / stream_destroy / sync / malloc / pinned, and the copy seam: work runs when its stream is synchronised."""

    def __init__(self):
        self.bufs, self.queues, self.destroyed = [], {}, {}

    def stream_create(self):
        s = len(self.queues) + 1
        self.queues[s], self.destroyed[s] = [], 0
        return s

    def stream_destroy(self, s):
        assert not self.queues[s], "a stream is destroyed with work in flight"
        self.destroyed[s] += 1

    def launch(self, s, fn, touched):
        assert not self.destroyed[s]
        for b in touched:
            b.stream = s
        self.queues[s].append(fn)

    def sync(self, s):
        for fn in self.queues[s]:
            fn()
        self.queues[s] = []
        for b in self.bufs:
            if b.stream == s:
                b.stream = None

    def malloc(self, nbytes):
        self.bufs.append(_Buf((nbytes,), False))
        return self.bufs[-1]

    def pinned(self, shape, dtype):
        assert np.dtype(dtype) == np.uint8
        self.bufs.append(_Buf(shape, True))
        return self.bufs[-1]

    def copy(self, ctx, kind, dst, src, nbytes, stream):
        assert ctx is self and kind in ("h2d", "d2h")
        pinned, device = (src, dst) if kind == "h2d" else (dst, src)
        assert isinstance(pinned.array, _Tracked) and not isinstance(device.array, _Tracked)

        def run():
            dst.bytes()[:nbytes] = src.bytes()[:nbytes]

        self.launch(stream, run, [pinned])

    def released_once(self):
        return all(b.freed == 1 for b in self.bufs) and all(v == 1 for v in self.destroyed.values())


class _Source:
    yuv_hw = scale = transfer = yuv_pix_fmt = None

    def __init__(self, name, seed, length, bad_at=None):
        self.read_path, self.seed, self.length, self.bad_at = name, seed, length, bad_at
        self.next, self.last_index, self.closed = 0, -1, 0

    def get_image(self):
        if self.next >= self.length:
            return None
        self.last_index, self.next = self.next, self.next + 1
        f = _frame(self.seed, self.last_index)
        return f.astype(np.float32) if self.last_index == self.bad_at else f

    def close(self):
        self.closed += 1


class _Rig:
    """A run of stream_pairs over two fake sources: the generator, the fake context and what the command side saw."""

    def __init__(self, monkeypatch, la, lb, batch, depth, bad_at=None, fail_at_call=None):
        self.ctx, self.info = _Ctx(), {}
        self.sources = {"A": _Source("A", 1, la, bad_at), "B": _Source("B", 101, lb)}
        self.views, self.calls, self.sizes = [], 0, []
        monkeypatch.setattr(pairs, "get_context", lambda: self.ctx)
        monkeypatch.setattr(pairs, "copy", self.ctx.copy)
        monkeypatch.setattr(pairs, "open_source", lambda args, path: (self.sources[path], (H, W) if self.sources[path].length else None))
        args = types.SimpleNamespace(a="A", b="B", batch=batch, depth=depth)

        def prepare(h, w):
            self.sizes.append((h, w))

            def enqueue(k, n, stream, sides, outs):
                self.calls += 1
                if self.calls == fail_at_call:
                    raise RuntimeError("launch failed")
                a, b, out = sides[0].d_rgb[k], sides[1].d_rgb[k], outs[0]

                def run():
                    out.array[: n * UNIT] = a.array[: n * UNIT] ^ b.array[: n * UNIT]

                self.ctx.launch(stream, run, [])

            def harvest(n, arrays):
                assert arrays[1] is None  # the output that is not downloaded has no staging
                self.views.append(arrays[0].data[0])  # a view of the staging, to show that it is reused
                return [np.array(arrays[0][j]).reshape(H, W, 3) for j in range(n)]

            return [(UNIT, True), (4, False)], enqueue, harvest

        self.gen = pairs.stream_pairs(args, self.info, "pairs-test", prepare)

    def released(self):
        return self.ctx.released_once() and all(s.closed == 1 for s in self.sources.values())


def _want(i):
    return _frame(1, i) ^ _frame(101, i)


@pytest.mark.parametrize("batch,depth,lengths", list(itertools.product((1, 3, 4), (1, 2, 3), ((0, 0), (0, 2), (4, 4), (8, 8), (9, 7), (7, 9)))))
def test_items_come_in_frame_order_with_the_right_contents(monkeypatch, batch, depth, lengths):
    la, lb = lengths
    rig = _Rig(monkeypatch, la, lb, batch, depth)
    items = list(rig.gen)  # every item is held until the end: a view of staging that a later batch overwrote would show here
    assert len(items) == min(la, lb)
    for i, item in enumerate(items):
        assert item.dtype == np.uint8 and np.array_equal(item, _want(i)), i
    assert rig.info.get("longer") == (None if la == lb else ("A" if la > lb else "B"))
    assert rig.sizes == ([(H, W)] if la and lb else [])  # prepare runs once, and not at all for an empty input
    # one launch per batch of the common prefix; a prefix that ends on a full batch costs an empty turn, not a launch
    assert rig.calls == -(-min(la, lb) // batch)
    assert len(rig.ctx.queues) == (depth if la and lb else 0)  # --depth buffer sets, a stream each
    assert rig.released()


def test_no_depth_means_two_buffer_sets(monkeypatch):
    rig = _Rig(monkeypatch, 4, 4, 2, None)
    assert len(list(rig.gen)) == 4 and len(rig.ctx.queues) == 2 and rig.released()


def test_items_are_copies_of_staging_that_is_reused(monkeypatch):
    rig = _Rig(monkeypatch, 8, 8, 1, 1)
    first = next(rig.gen)
    assert np.array_equal(first, _want(0)) and np.array_equal(rig.views[0].reshape(H, W, 3), first)
    rest = list(rig.gen)
    assert len(rest) == 7 and all(v.base is rig.views[0].base for v in rig.views)  # one set: every batch went through the same staging
    assert not np.array_equal(rig.views[0].reshape(H, W, 3), _want(0))  # ... which a later batch overwrote
    assert np.array_equal(first, _want(0))  # while the item held since then is what it was


def test_a_normal_end_releases_everything_once(monkeypatch):
    rig = _Rig(monkeypatch, 9, 7, 4, 2)
    assert len(list(rig.gen)) == 7 and rig.ctx.bufs and rig.released()


def test_a_systemexit_out_of_fill_releases_everything_once(monkeypatch):
    rig = _Rig(monkeypatch, 9, 9, 4, 2, bad_at=5)
    got = []
    with pytest.raises(SystemExit) as e:
        for item in rig.gen:
            got.append(item)
    assert str(e.value) == f"pairs-test: A: frame 5 is float32 {(H, W, 3)}, not uint8 {(H, W, 3)}"  # the command that ran is named
    assert len(got) == 0  # frames 0..3 were in flight on the other set when frame 5 was read
    assert rig.ctx.bufs and rig.released()


def test_an_exception_out_of_enqueue_releases_everything_once(monkeypatch):
    rig = _Rig(monkeypatch, 9, 9, 2, 3, fail_at_call=3)
    with pytest.raises(RuntimeError, match="launch failed"):
        list(rig.gen)
    assert rig.ctx.bufs and rig.released()


def test_closing_the_generator_after_the_first_item_releases_everything_once(monkeypatch):
    rig = _Rig(monkeypatch, 9, 9, 3, 2)
    assert np.array_equal(next(rig.gen), _want(0))
    assert not rig.released() and any(rig.ctx.queues.values())  # the second batch is in flight
    rig.gen.close()
    assert rig.released() and not any(rig.ctx.queues.values())


def test_frame_sizes_that_differ_are_refused_before_any_allocation(monkeypatch):
    rig = _Rig(monkeypatch, 2, 2, 2, 2)
    monkeypatch.setattr(pairs, "open_source", lambda args, path: (rig.sources[path], (H, W) if path == "A" else (H, W + 2)))
    with pytest.raises(SystemExit) as e:
        list(rig.gen)
    assert str(e.value) == f"pairs-test: frame sizes differ: A is {W}x{H}, B is {W + 2}x{H}"
    assert not rig.ctx.bufs and not rig.ctx.queues and all(s.closed == 1 for s in rig.sources.values())
