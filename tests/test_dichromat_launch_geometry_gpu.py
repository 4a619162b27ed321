"""The marching-strip dichromat kernel at every launch geometry its host code can choose, bit-exact against the oracle.

The first call for a (radius, type, batch, frame size) picks the workgroup width (NG = 64: wave-specialised, or 128), the row
chunks per strip and, for float32 NG = 64, full or narrowed strips by timing them; a run of the rest of the suite sees one
choice.  Here every choice is pinned (AVX_MARCH_NG / AVX_MARCH_CHUNKS / AVX_MARCH_SWCAP, which the library reads on every
call), DichromatOp.last_launch() must report exactly the pinned geometry -- so a pin that did not take, or a shape that fell
through to another kernel, fails instead of passing empty -- and the bytes must equal oracle.dichromat_visualize, which runs
ONCE per (spec, frame).  No device result is compared with another device result only.  Only geometries the unpinned host
code can reach are pinned (the float32 kernel stores 16-byte row vectors; other strip widths are not its contract):
chunks 5 and H // 32 stand for values of the fallback ceil(resident workgroups / (frames x strips)).

The tuner itself (a fresh context under AVX_MARCH_NOSEED) and its table (more shapes than it used to hold) are at the end."""
import dataclasses

import numpy as np
import pytest

import _march_geometry as G

pytestmark = pytest.mark.gpu

# one spec per marching instantiation: key -> (species, sigma override, R, float64)
SPECS = {
    "r1": ("squirrel", 0.3, 1, False),       # cv_auto_ksize(0.3) == 3: no species has it
    "squirrel": ("squirrel", None, 3, False),
    "cat": ("cat", None, 4, True),
    "lion": ("lion", None, 5, False),
    "wolf": ("wolf", None, 6, False),
    "bear": ("bear", None, 7, False),
    "raccoon": ("raccoon", None, 8, False),
    "r9": ("raccoon", 2.25, 9, False),       # cv_auto_ksize(2.25) == 19: no species has it
    "dog": ("dog", None, 14, False),
}
CHUNKS = (1, 2, 3, 5, 8, 24)  # and H // 32, the most the host code allows

CASES = []   # (spec, frame, NG, narrow, nchunks) of every pinned launch compared with the oracle
PICKS = {}   # spec -> what the unseeded tuner picked at 1080p


@pytest.fixture(scope="module")
def av():
    import animal_vision_amd as av

    assert av.device_count() > 0, "no GPU visible"
    return av


class _Device:
    """Frames uploaded once and reused across geometries; the output buffer is poisoned before every launch, so bytes a
    launch did not write cannot pass as the (identical) result of the launch before it."""

    def __init__(self):
        self.bufs = {}

    def run(self, op, fkey, batch):
        ctx = op._ctx()
        if (id(ctx), fkey) not in self.bufs:
            self.bufs[(id(ctx), fkey)] = (ctx.upload(batch), ctx.malloc(batch.nbytes), np.full(batch.shape, 0xA5, np.uint8))
        d_in, d_out, poison = self.bufs[(id(ctx), fkey)]
        ctx.upload(poison, d_out)
        n, H, W, _ = batch.shape
        op.run_device(d_in, d_out, n, H, W)
        return ctx.download(d_out, batch.shape, np.uint8)

    def drop(self, ctx=None):
        for k in [k for k in self.bufs if ctx is None or k[0] == id(ctx)]:
            d_in, d_out, _ = self.bufs.pop(k)
            d_in.free()
            d_out.free()


@pytest.fixture(scope="module")
def dev():
    d = _Device()
    yield d
    d.drop()
    print(f"\n[geometry] {len(CASES)} pinned (spec, frame, geometry) launches compared with the oracle")
    for k, v in PICKS.items():
        print(f"[geometry] unseeded tuner at 1080p, {k}: {v}")


def _specs(av, oracle, key):
    """(product spec, oracle spec, R, f64) of one sweep spec; sigma overridden on both sides for the R = 1 / R = 9 kernels."""
    from animal_vision_amd import animals
    from animal_vision_amd.dichromat import cv_auto_ksize

    name, sigma, R, f64 = SPECS[key]
    ps, os_ = getattr(animals, name.capitalize()).SPEC, oracle.DICHROMATS[name]
    if sigma is not None:
        ps, os_ = dataclasses.replace(ps, sigma=sigma), dataclasses.replace(os_, sigma=sigma)
    assert ps.sigma == os_.sigma and cv_auto_ksize(ps.sigma) // 2 == R and (ps.color == "cat_merge") == f64
    return ps, os_, R, f64


_OPS = {}


def _op(av, oracle, key, ctx=None):
    from animal_vision_amd.dichromat import DichromatOp

    if ctx is not None:
        return DichromatOp(_specs(av, oracle, key)[0], ctx)
    if key not in _OPS:
        _OPS[key] = DichromatOp(_specs(av, oracle, key)[0])
    return _OPS[key]


def _want(oracle, av, key, fkey, batch):
    """The oracle's bytes for every frame of the batch: one oracle run per (spec, frame), kept for the session."""
    os_ = _specs(av, oracle, key)[1]
    return np.stack([G.oracle_bytes(oracle, key, os_, fkey + (i,) if batch.shape[0] > 1 else fkey, batch[i]) for i in range(batch.shape[0])])


def _pin(monkeypatch, NG, chunks, swcap):
    G.unset_march_pins(monkeypatch)
    monkeypatch.setenv("AVX_MARCH_NG", str(NG))
    monkeypatch.setenv("AVX_MARCH_CHUNKS", str(chunks))
    if swcap:
        monkeypatch.setenv("AVX_MARCH_SWCAP", str(swcap))


def _check_launch(op, want, what):
    li = op.last_launch()
    got = {k: li[k] for k in want}
    assert got == want, f"{what}: the pinned geometry did not run: reported {li}, intended {want}"
    assert li["tuned_now"] == 0, f"{what}: a pinned launch ran the timing pass: {li}"
    return li


def _sweep(monkeypatch, av, oracle, dev, key, fkey, batch, NGs=(64, 128), chunks=None):
    """Every (NG, strip width, chunks) the host code can choose for this batch; returns the reported launches."""
    _, _, R, f64 = _specs(av, oracle, key)
    n, H, W, _ = batch.shape
    assert (n * H * W * 3) % 4 == 0 and H >= 2 * (R + 4), "the marching kernel does not take this batch"
    want = _want(oracle, av, key, fkey, batch)
    op = _op(av, oracle, key)
    launches = []
    for NG in NGs:
        nw = G.narrowed_width(R, f64, NG)
        for narrow in ((False, True) if nw and W > nw else (False,)):  # launch_march: `if (a.W <= sw_narrow) sw_narrow = 0`
            seen = set()
            for c in (chunks or CHUNKS + (H // 32,)):
                exp = G.expected_launch(R, f64, NG, n, H, W, c, narrow)
                if (exp["nchunks"], exp["ch"]) in seen:  # clamped to a split already run
                    continue
                seen.add((exp["nchunks"], exp["ch"]))
                _pin(monkeypatch, NG, c, nw if narrow else 0)
                got = dev.run(op, fkey, batch)
                what = f"{key} {n}x{H}x{W} NG={NG} chunks={c}{' narrowed strips' if narrow else ''}"
                li = _check_launch(op, exp, what)
                G.assert_same_bytes(got, want, what, li)
                launches.append(li)
                CASES.append((key, fkey, NG, narrow, exp["nchunks"]))
    G.unset_march_pins(monkeypatch)
    print(f"[geometry] {key} {n}x{H}x{W}: {len(launches)} geometries bit-exact; {len(CASES)} so far")
    return launches


def _frame(seed, H, W):
    return (seed, H, W), G.frame(seed, H, W)[None]


@pytest.mark.parametrize("key", list(SPECS))
def test_1080p_every_geometry(av, oracle, dev, monkeypatch, key):
    fkey, batch = _frame(G.SEED_1080P, 1080, 1920)
    launches = _sweep(monkeypatch, av, oracle, dev, key, fkey, batch)
    f64 = SPECS[key][3]
    assert {(l["NG"], l["spec"]) for l in launches} == {(64, 1), (128, 0)}
    assert any(l["narrow"] for l in launches) == (not f64)
    for NG in (64, 128):  # 24 requested chunks are 23 of 48 rows; H // 32 = 33 requested are 30 of 36 rows
        assert {l["nchunks"] for l in launches if l["NG"] == NG and not l["narrow"]} == {1, 2, 3, 5, 8, 23, 30}


@pytest.mark.parametrize("key", ["dog", "cat", "squirrel"])
def test_4k_every_geometry(av, oracle, dev, monkeypatch, key):
    fkey, batch = _frame(G.SEED_4K, 2160, 3840)
    launches = _sweep(monkeypatch, av, oracle, dev, key, fkey, batch)
    assert max(l["nchunks"] for l in launches) == G.set_chunks(2160, 2160 // 32)[0]


@pytest.mark.parametrize("key", list(SPECS))
def test_720p_both_xcd_remaps_for_both_widths(av, oracle, dev, monkeypatch, key):
    """xcd_remap follows from the workgroup count (% 8 == 0) and changes which workgroup gets which strip: at 1280 px
    every instantiation has a strip count that gives 0 with one chunk and 1 with eight."""
    fkey, batch = _frame(21, 720, 1280)
    launches = _sweep(monkeypatch, av, oracle, dev, key, fkey, batch)
    for NG in (64, 128):
        full = {l["nchunks"]: l for l in launches if l["NG"] == NG and not l["narrow"]}
        assert full[1]["nstrips"] > 1 and full[1]["xcd_remap"] == 0 and full[8]["xcd_remap"] == 1, (key, NG, full)


@pytest.mark.parametrize("H,last", [(1057, 1), (1059, 3), (1061, 5)])
@pytest.mark.parametrize("key", list(SPECS))
def test_last_chunk_of_1_3_5_rows(av, oracle, dev, monkeypatch, key, H, last):
    """24 chunks of 48 rows: 22 full ones and a last chunk of 1, 3 or 5 rows (fewer than one 4-row iteration, fewer than the
    2R priming rows); the other splits of these odd heights run as well."""
    fkey, batch = _frame(22, H, 1920)
    launches = _sweep(monkeypatch, av, oracle, dev, key, fkey, batch)
    l24 = [l for l in launches if l["nchunks"] == 23]
    assert len(l24) >= 2 and all(l["ch"] == 48 and G.last_chunk_rows(H, l["nchunks"], l["ch"]) == last for l in l24)


@pytest.mark.parametrize("key", list(SPECS))
def test_last_strip_of_one_pixel(av, oracle, dev, monkeypatch, key):
    """W = 1921 at 1080 rows: the 2-columns-per-thread float32 kernels get 16 strips of 128 px, the last 1 px wide (NG = 64),
    or 8 of 256 with a last strip of 129 px (NG = 128); the 4-columns-per-thread kernels (R = 1, 3) get their 1-px strip at
    W = 3841 = 15 * 256 + 1."""
    _, _, R, f64 = _specs(av, oracle, key)
    xpt = G.march_cfg(R, f64, 64)[0]
    H, W = (1080, 1921) if xpt == 2 else (64, 3841)
    fkey, batch = _frame(23, H, W)
    launches = _sweep(monkeypatch, av, oracle, dev, key, fkey, batch)
    tails = {(l["NG"], l["narrow"]): G.last_strip_px(W, l["nstrips"], l["sw"]) for l in launches}
    if not f64:
        assert tails[(64, 0)] == 1, tails
    if xpt == 2:
        assert tails[(128, 0)] == 129, tails
    if xpt == 4:  # and the same kernels at W = 1921 (8 strips of 256, the last 129 px)
        fkey, batch = _frame(23, 1080, 1921)
        launches = _sweep(monkeypatch, av, oracle, dev, key, fkey, batch, chunks=(1, 3, 8))
        assert all(G.last_strip_px(1921, l["nstrips"], l["sw"]) == 129 for l in launches if l["NG"] == 64 and not l["narrow"])


@pytest.mark.parametrize("key", list(SPECS))
def test_narrow_and_short_frames(av, oracle, dev, monkeypatch, key):
    """A frame narrower than one strip (one ragged strip, every column reflects on both sides for the wide radii), and the
    shortest frame the kernel takes, H = 2 (R + 4), where every row chunk request clamps to one chunk."""
    R = SPECS[key][2]
    fkey, batch = _frame(24, 256, 52)
    launches = _sweep(monkeypatch, av, oracle, dev, key, fkey, batch)
    assert all(l["nstrips"] == 1 and l["sw"] == 64 for l in launches) and {l["nchunks"] for l in launches} == {1, 2, 3, 5, 8}
    fkey, batch = _frame(25, 2 * (R + 4), 1920)
    launches = _sweep(monkeypatch, av, oracle, dev, key, fkey, batch)
    assert launches and all(l["nchunks"] == 1 for l in launches)


def test_cat_strips_that_are_no_multiple_of_16(av, oracle, dev, monkeypatch):
    """The cat's wave-specialised form caps strips at 120 px: W = 354 gives three 118-px strips (from W, not from a knob)."""
    fkey, batch = _frame(26, 128, 354)
    launches = _sweep(monkeypatch, av, oracle, dev, "cat", fkey, batch)
    assert {(l["nstrips"], l["sw"]) for l in launches if l["NG"] == 64} == {(3, 118)}


@pytest.mark.parametrize("key", list(SPECS))
def test_batch_with_dark_frames(av, oracle, dev, monkeypatch, key):
    """4 x 540 x 960: frames 1 and 3 have no byte above 1 (not divided by 255: the per-frame fix-up launch, same chunked
    geometry), frame 2 is such a frame plus one byte 2, which makes it an ordinary frame; flags are per frame."""
    rng = np.random.default_rng(27)
    batch = rng.integers(0, 256, (4, 540, 960, 3), dtype=np.uint8)
    batch[1:] = rng.integers(0, 2, (3, 540, 960, 3), dtype=np.uint8)
    batch[2, 300, 500, 1] = 2
    assert batch[1].max() == 1 and batch[3].max() == 1 and batch[2].max() == 2 and (batch[2] > 1).sum() == 1
    launches = _sweep(monkeypatch, av, oracle, dev, key, (27, 540, 960), batch)
    assert {l["nchunks"] for l in launches} >= {1, 2, 3, 5, 8}


def test_seeded_wolf_batch_runs_the_narrowed_strips(av, oracle, dev, monkeypatch):
    """The narrowed width restated in _march_geometry.narrowed_width against a tuned call: the seeded table holds wolf
    32 x 1080p as NG = 64, 8 chunks, narrowed strips -- nothing pinned here."""
    G.unset_march_pins(monkeypatch)
    fkey, one = _frame(G.SEED_1080P, 1080, 1920)
    want = _want(oracle, av, "wolf", fkey, one)
    op = _op(av, oracle, "wolf")
    got = dev.run(op, ("x32",) + fkey, np.repeat(one, 32, axis=0))
    li = op.last_launch()
    exp = G.expected_launch(6, False, 64, 32, 1080, 1920, 8, narrow=True)
    assert exp["sw"] == 112 and {k: li[k] for k in exp} == exp and li["tuned_now"] == 0, li
    G.assert_same_bytes(got, np.repeat(want, 32, axis=0), "wolf 32 x 1080p, seeded geometry", li)


# ---- the tuner ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(SPECS))
def test_unseeded_tuner_first_and_second_call(av, oracle, dev, monkeypatch, key):
    """A fresh context that measures everything: the first call times every candidate while writing the caller's output
    buffer and must leave the oracle's bytes there; the second call reuses what the first remembered; the same geometry
    pinned gives the same bytes."""
    G.unset_march_pins(monkeypatch)
    monkeypatch.setenv("AVX_MARCH_NOSEED", "1")
    _, _, R, f64 = _specs(av, oracle, key)
    fkey, batch = _frame(G.SEED_1080P, 1080, 1920)
    want = _want(oracle, av, key, fkey, batch)
    ctx = av.Context(0)
    try:
        op = _op(av, oracle, key, ctx)
        got = dev.run(op, fkey, batch)
        first = op.last_launch()
        assert first["family"] == "march" and first["tuned_now"] == 1 and (first["R"], first["f64"]) == (R, int(f64)), first
        G.assert_same_bytes(got, want, f"{key} 1080p, first (tuning) call", first)
        got = dev.run(op, fkey, batch)
        second = op.last_launch()
        assert second == dict(first, tuned_now=0), (first, second)
        G.assert_same_bytes(got, want, f"{key} 1080p, second call", second)
        # what it picked is a geometry this file pins: the reported numbers follow from (NG, chunks, narrow) by the host formulas
        exp = G.expected_launch(R, f64, first["NG"], 1, 1080, 1920, first["nchunks"], bool(first["narrow"]))
        assert {k: first[k] for k in exp} == exp, (first, exp)
        _pin(monkeypatch, first["NG"], first["nchunks"], G.narrowed_width(R, f64, first["NG"]) if first["narrow"] else 0)
        got = dev.run(op, fkey, batch)
        pinned = _check_launch(op, exp, f"{key} 1080p pinned to the tuner's pick")
        G.assert_same_bytes(got, want, f"{key} 1080p pinned to the tuner's pick", pinned)
        PICKS[key] = {k: first[k] for k in ("R", "f64", "NG", "nchunks", "ch", "sw", "nstrips", "narrow", "xcd_remap")}
        print(f"[geometry] unseeded tuner at 1080p, {key}: {PICKS[key]}")
    finally:
        dev.drop(ctx)
        ctx.close()


def _shape_run(av, oracle, dev, op, key, n, H, W, seed, check=True):
    one_key, one = _frame(seed, H, W)
    got = dev.run(op, (n,) + one_key, np.repeat(one, n, axis=0))
    li = op.last_launch()
    assert li["family"] == "march", li
    if check:
        G.assert_same_bytes(got, np.repeat(_want(oracle, av, key, one_key, one), n, axis=0), f"{key} {n}x{H}x{W}", li)
    return li


def test_tuner_table_holds_24_shapes(av, oracle, dev, monkeypatch):
    """24 distinct measured shapes (batches of 1..24 frames of 512 x 512) in one context: each is measured once, on its first
    call, and never again.  The table used to be 64 entries with 14 seeded and 3 per shape, and a result that did not fit
    was dropped: from about the 17th shape on every call ran the whole timing pass again."""
    G.unset_march_pins(monkeypatch)
    ctx = av.Context(0)
    try:
        op = _op(av, oracle, "wolf", ctx)
        for n in range(1, 25):
            li = _shape_run(av, oracle, dev, op, "wolf", n, 512, 512, 31)
            assert li["tuned_now"] == 1, (n, li)
        again = [_shape_run(av, oracle, dev, op, "wolf", n, 512, 512, 31) for n in range(1, 25)]
        assert [n for n, li in zip(range(1, 25), again) if li["tuned_now"]] == [], "shapes measured again on their second call"
    finally:
        dev.drop(ctx)
        ctx.close()


def test_tuner_table_overflow_drops_the_oldest_shape_and_keeps_the_seeds(av, oracle, dev, monkeypatch):
    """More measured shapes than the table holds (csrc/avx_internal.h: 128 entries, 14 of them seeded, 3 per shape -> 38
    shapes): the newest stay remembered, the oldest shape is measured again when it comes back (its width and chunk entries
    leave together), and the seeded entries survive (dog 32 x 1080p: NG = 64, 4 chunks, no timing pass)."""
    G.unset_march_pins(monkeypatch)
    ctx = av.Context(0)
    try:
        op = _op(av, oracle, "wolf", ctx)
        heights = [512 + 4 * i for i in range(44)]
        for i, H in enumerate(heights):
            li = _shape_run(av, oracle, dev, op, "wolf", 1, H, 512, 32, check=i in (0, 43))
            assert li["tuned_now"] == 1, (H, li)
        for H in heights[-20:]:
            assert _shape_run(av, oracle, dev, op, "wolf", 1, H, 512, 32, check=False)["tuned_now"] == 0, H
        assert _shape_run(av, oracle, dev, op, "wolf", 1, heights[0], 512, 32)["tuned_now"] == 1, "the oldest shape was not evicted: the table did not fill"
        assert _shape_run(av, oracle, dev, op, "wolf", 1, heights[0], 512, 32)["tuned_now"] == 0
        dog = _op(av, oracle, "dog", ctx)
        li = _shape_run(av, oracle, dev, dog, "dog", 32, 1080, 1920, G.SEED_1080P, check=False)
        exp = G.expected_launch(14, False, 64, 32, 1080, 1920, 4)
        assert li["tuned_now"] == 0 and {k: li[k] for k in exp} == exp, li
    finally:
        dev.drop(ctx)
        ctx.close()
