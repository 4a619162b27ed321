"""GPU: the wide view of the dichromats (csrc/dichromat_wide.hip).

  * avx_dichromat_wide_u8 under either route (AVX_WIDE_ROUTE=fused|planes) against the chain that defines it for the Gaussian,
    row-gain and plain descriptors, frame by frame: avx_binocular_warp_u8 -> float32 frame -> avx_dichromat_u8(in_f32 = 1).  Identical
    bytes.  The chain exists at the parent commit; the new code is never compared against itself.
  * batches: per-frame "any byte > 1" flags, fewer frames than the buffers hold, batch 1 / 5 / 16, the group walk of the planes route.
  * all 20 species and three geometries against the oracle composition of tests/_wide_ref.py -- the streak species have no chain --
    under the float pipelines' contract, tests/_sensitivity.check_codes at its default caps; the baseline byte for byte.
  * night= and AutoNight with fov=, Cat with fov=, the stream operator, the `video` command, the entry's refusals and its ordering
    on a stream without synchronisation."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _daynight_ref as DN
import _night_ref as N
import _wide_ref as WR
import _yuv_ref as R
from _sensitivity import check_codes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIES = ["dog", "cat", "sheep", "pig", "cow", "goat", "horse", "rabbit", "panda", "deer", "kangaroo", "rat", "squirrel", "elephant", "lion",
           "tiger", "bear", "wolf", "fox", "raccoon"]
# (H, W): smaller than every halo, several reflections; no multiple of a tile, a vector or 4; several tiles, odd width; exact tile multiples
SIZES = [(6, 5), (37, 53), (70, 131), (96, 160)]
ROUTES = ["fused", "planes"]


@pytest.fixture(scope="module")
def G():
    from animal_vision_amd import geometry

    return geometry


@pytest.fixture(scope="module")
def ctx():
    from animal_vision_amd.runtime import get_context

    return get_context()


def _spec(name):
    """The descriptor cases of the chain tests: Dog r = 14, Raccoon r = 8, Squirrel r = 3, Rat (row gain, r = 0), no post stage,
    Gaussian + chroma compression."""
    from animal_vision_amd import animals
    from animal_vision_amd.dichromat import DichromatSpec

    if name == "none":
        return DichromatSpec("plain", 0.58, 0.9, post="none")
    if name == "gauss+chroma":
        return DichromatSpec("soft", 0.6, 0.95, sigma=1.2, chroma=0.06)
    if name == "rowgain+chroma":
        return DichromatSpec("ratty", 0.05, 0.86, post="scone", chroma=0.06)
    return getattr(animals, name).SPEC


def _fov(geometry, ratio=1.30):
    from animal_vision_amd.dichromat import FovSpec

    phi, overlap, camera = geometry
    return FovSpec(phi, overlap, camera, ratio)


def _animal(name, geometry, night=None):
    from animal_vision_amd import animals

    return getattr(animals, name.capitalize())(fov=_fov(geometry), night=night)


def _tables(G, H, W, geometry):
    phi, overlap, camera = geometry
    return G.binocular_warp_tables(H, W, W, H, camera, phi, overlap)


def _noise(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


_CHAINS = {}


def _chain(G, ctx, frames, spec, geometry, key=None):
    """The definition: per frame avx_binocular_warp_u8 into a float32 frame, then avx_dichromat_u8 with in_f32 = 1.  key: computed once."""
    from animal_vision_amd.dichromat import DichromatOp

    if key is not None and key in _CHAINS:
        return _CHAINS[key]
    n, H, W, _ = frames.shape
    op = DichromatOp(spec, ctx)
    tables = _tables(G, H, W, geometry)
    d_in, d_warp, d_out = ctx.malloc(H * W * 3), ctx.malloc(H * W * 3 * 4), ctx.malloc(H * W * 3)
    out = np.empty_like(frames)
    try:
        op.desc.in_f32 = 1
        for f in range(n):
            ctx.upload(frames[f], d_in)
            G.binocular_warp_device(ctx, d_in, H, W, tables, H, W, d_warp)
            op.run_device(d_warp, d_out, 1, H, W)
            out[f] = ctx.download(d_out, (H, W, 3), np.uint8)
    finally:
        d_in.free(); d_warp.free(); d_out.free()
    out.setflags(write=False)
    if key is not None:
        _CHAINS[key] = out
    return out


def _entry(G, ctx, frames, spec, geometry, capacity=None):
    """avx_dichromat_wide_u8 over the first len(frames) frames of buffers that hold `capacity`; returns the whole output buffer."""
    from animal_vision_amd.dichromat import DichromatOp

    n, H, W, _ = frames.shape
    cap = capacity or n
    op = DichromatOp(spec, ctx)
    op.prepare_tables(H)
    tab, ptrs = G.binocular_warp_tables_device(ctx, _tables(G, H, W, geometry))
    host = np.full((cap, H, W, 3), 0xA5, np.uint8)
    host[:n] = frames
    d_in, d_out = ctx.upload(host), ctx.upload(np.full((cap, H, W, 3), 0x5A, np.uint8))
    try:
        G.dichromat_wide_device(ctx, d_in, d_out, n, H, W, op.desc, ptrs)
        return ctx.download(d_out, (cap, H, W, 3), np.uint8)
    finally:
        d_in.free(); d_out.free(); tab.free()


def _same(got, want, what):
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]])


def _geometry_for(H, W, k=0):
    """The tiny frame is black under the narrow camera (and nearly so under Cat's): it always gets the two-eye geometry."""
    return WR.TWO_EYES if min(H, W) < 13 else WR.GEOMETRIES[k % 3]


# ---------------------------------------------------------------- either route against the chain ----------------------------------
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("name", ["Dog", "Raccoon", "Squirrel", "Rat", "none", "gauss+chroma", "rowgain+chroma"])
def test_both_routes_equal_the_chain(G, ctx, monkeypatch, name, H, W):
    spec = _spec(name)
    for k in range(1 if min(H, W) < 13 else 3):
        geometry = _geometry_for(H, W, k + len(name))
        frames = _noise(H + W + k, 1, H, W, 3)
        want = _chain(G, ctx, frames, spec, geometry)
        assert want.max() > 64, (name, H, W, geometry)  # lit columns: a black frame would pass anything
        for route in ROUTES:
            monkeypatch.setenv("AVX_WIDE_ROUTE", route)
            _same(_entry(G, ctx, frames, spec, geometry), want, (name, H, W, geometry, route))
        monkeypatch.delenv("AVX_WIDE_ROUTE")
        _same(_entry(G, ctx, frames, spec, geometry), want, (name, H, W, geometry, "default route"))


def test_the_fused_kernel_at_other_tiles(G, ctx, monkeypatch):
    """AVX_WIDE_TILE: a tile smaller than the halo, one wider than the frame, one whose LDS need makes the host halve it."""
    H, W = 70, 131
    frames = _noise(11, 1, H, W, 3)
    monkeypatch.setenv("AVX_WIDE_ROUTE", "fused")
    for name in ("Dog", "gauss+chroma", "Rat"):
        want = _chain(G, ctx, frames, _spec(name), WR.TWO_EYES)
        for tile in ("8x4", "64x32", "256x64", "256x256"):
            monkeypatch.setenv("AVX_WIDE_TILE", tile)
            _same(_entry(G, ctx, frames, _spec(name), WR.TWO_EYES), want, (name, tile))
        monkeypatch.delenv("AVX_WIDE_TILE")


def test_structured_content_equals_the_chain(G, ctx, monkeypatch):
    from animal_vision_amd.synthetic import structured_frame

    frames = np.stack([structured_frame(5, 70, 131), structured_frame(6, 70, 131)])
    for name in ("Dog", "Rat"):
        want = _chain(G, ctx, frames, _spec(name), WR.CAT_GEOMETRY)
        for route in ROUTES:
            monkeypatch.setenv("AVX_WIDE_ROUTE", route)
            _same(_entry(G, ctx, frames, _spec(name), WR.CAT_GEOMETRY), want, (name, route))


# ---------------------------------------------------------------- batches ---------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_dark_frame_in_the_middle_of_a_batch(G, ctx, monkeypatch, route):
    """A frame whose bytes are all 0 or 1 is not divided by 255 (get_normalized_image); in a batch that is decided frame by frame."""
    H, W = 37, 53
    monkeypatch.setenv("AVX_WIDE_ROUTE", route)
    bright = _noise(2, 4, H, W, 3)
    dark = _noise(1, H, W, 3) & 1
    batch = np.stack([bright[0], bright[1], dark, bright[2], bright[3]])
    for name in ("Raccoon", "Rat"):
        want = _chain(G, ctx, batch, _spec(name), WR.TWO_EYES, key=("dark", name))
        assert want[2].max() > 2  # a 1 is 1.0 here; divided by 255 it would be 3e-4 linear
        _same(_entry(G, ctx, batch, _spec(name), WR.TWO_EYES), want, (name, "bright, bright, dark, bright, bright"))
        _same(_entry(G, ctx, batch[2:3], _spec(name), WR.TWO_EYES), want[2:3], (name, "dark alone"))


@pytest.mark.parametrize("route", ROUTES)
def test_fewer_frames_than_the_buffers_hold(G, ctx, monkeypatch, route):
    H, W = 37, 53
    monkeypatch.setenv("AVX_WIDE_ROUTE", route)
    frames = _noise(7, 2, H, W, 3)
    got = _entry(G, ctx, frames, _spec("Squirrel"), WR.TWO_EYES, capacity=4)
    _same(got[:2], _chain(G, ctx, frames, _spec("Squirrel"), WR.TWO_EYES, key="fewer"), "n = 2 of 4")
    assert (got[2:] == 0x5A).all()  # the frames beyond n_frames are not written


@pytest.mark.parametrize("route", ROUTES)
def test_a_frames_bytes_do_not_depend_on_the_batch(G, ctx, monkeypatch, route):
    H, W = 37, 53
    monkeypatch.setenv("AVX_WIDE_ROUTE", route)
    frames = _noise(9, 16, H, W, 3)
    frames[3] &= 1
    for name in ("Dog", "Rat"):
        want = _chain(G, ctx, frames, _spec(name), WR.CAT_GEOMETRY, key=("batch", name))
        _same(_entry(G, ctx, frames, _spec(name), WR.CAT_GEOMETRY), want, (name, 16))
        _same(_entry(G, ctx, frames[:5], _spec(name), WR.CAT_GEOMETRY), want[:5], (name, 5))
        for f in (0, 3, 15):
            _same(_entry(G, ctx, frames[f : f + 1], _spec(name), WR.CAT_GEOMETRY), want[f : f + 1], (name, 1, f))


_GROUP_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_wide_gpu as T
from animal_vision_amd import geometry as G
from animal_vision_amd.runtime import get_context
frames = np.load({frames!r})
for name in ("Dog", "Horse", "Rat"):
    np.save({out!r} + name + ".npy", T._entry(G, get_context(), frames, T._spec(name), T.WR.TWO_EYES))
print("walked")
"""


def test_group_walk_in_a_fresh_process(G, ctx, tmp_path):
    """A batch of 5 in groups of 2 on the planes route (AVX_WIDE_GROUP, read per call; set for a child so that no other test sees it)."""
    H, W = 37, 53
    frames = _noise(21, 5, H, W, 3)
    frames[1] &= 1
    np.save(str(tmp_path / "frames.npy"), frames)
    out = str(tmp_path / "group_")
    env = dict(os.environ, AVX_WIDE_GROUP="2", AVX_WIDE_ROUTE="planes")
    script = _GROUP_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), frames=str(tmp_path / "frames.npy"), out=out)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "walked" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    for name in ("Dog", "Rat"):
        _same(np.load(out + name + ".npy"), _chain(G, ctx, frames, _spec(name), WR.TWO_EYES), name)
    got = np.load(out + "Horse.npy")  # no chain: the same entry, frame by frame, in this process
    for f in range(5):
        _same(got[f : f + 1], _entry(G, ctx, frames[f : f + 1], _spec("Horse"), WR.TWO_EYES), ("Horse", f))


# ---------------------------------------------------------------- all 20 species against the oracle -------------------------------
ORACLE_CASES = [("noise", 13, 13), ("white", 13, 13), ("ramp", 37, 70), ("dark", 37, 70), ("ones", 37, 70), ("lamps", 96, 131), ("noise", 96, 131),
                ("black", 37, 70)]


def _check(oracle, name, frame, geometry, got, what, rod=None, bloom=0.0):
    sp = oracle.DICHROMATS[name]
    want = WR.wide_ref(sp, frame, geometry, rod=rod, bloom=bloom)
    check_codes(got, want, what, lambda seed: WR.wide_ref(sp, frame, geometry, rod=rod, bloom=bloom, jit=oracle.relative_jitter(seed)))
    return want


@pytest.mark.parametrize("name", SPECIES)
def test_all_species_against_the_oracle(oracle, name):
    assert len(oracle.DICHROMATS) == 20 and name in oracle.DICHROMATS
    for g, geometry in enumerate(WR.GEOMETRIES):
        animal = _animal(name, geometry)
        for kind, H, W in ORACLE_CASES:
            frame = N.frames(kind, H, W, seed=len(name) + g)
            base, out = animal.visualize(frame)
            assert out.dtype == np.uint8 and out.shape == frame.shape
            assert np.array_equal(base, WR.baseline(frame, geometry)), (name, geometry, kind, H, W)
            want = _check(oracle, name, frame, geometry, out, (name, geometry, kind, H, W))
            if kind == "black":
                assert not out.any()
            if kind == "noise" and WR.lit_columns(W, geometry).sum() >= 2:  # lit columns: the view is there, not a black frame
                assert want.max() > 64 and out.max() > 64, (name, geometry, kind, int(out.max()))


@pytest.mark.parametrize("name", ["rat", "horse", "dog"])
def test_one_animal_at_alternating_sizes(name):
    """The per-row host tables (row gains, streak taps) follow the frame's height when one animal's operators of several sizes take turns."""
    shared = _animal(name, WR.TWO_EYES)
    for H, W in [(37, 70), (96, 131), (37, 70), (13, 13), (96, 131)]:
        frame = N.frames("noise", H, W, seed=H)
        base, out = shared.visualize(frame)
        fbase, fout = _animal(name, WR.TWO_EYES).visualize(frame)
        _same(out, fout, (name, H, W))
        _same(base, fbase, (name, H, W, "baseline"))


@pytest.mark.parametrize("name", ["dog", "horse"])
def test_one_video_sized_frame(oracle, name):
    frame = N.frames("lamps", 270, 480)
    for geometry in (WR.CAT_GEOMETRY, WR.TWO_EYES):
        base, out = _animal(name, geometry).visualize(frame)
        assert np.array_equal(base, WR.baseline(frame, geometry))
        _check(oracle, name, frame, geometry, out, (name, geometry, "270 x 480"))


def test_the_streak_species_under_a_forced_route_stay_on_planes(G, ctx, monkeypatch, oracle):
    """AVX_WIDE_ROUTE=fused has no streak form: the entry keeps the planes route and its bytes."""
    frame = N.frames("noise", 37, 70)
    want = _entry(G, ctx, frame[None], _spec("Horse"), WR.TWO_EYES)
    monkeypatch.setenv("AVX_WIDE_ROUTE", "fused")
    _same(_entry(G, ctx, frame[None], _spec("Horse"), WR.TWO_EYES), want, "horse, fused asked")
    _check(oracle, "horse", frame, WR.TWO_EYES, want[0], "horse through the entry")


# ---------------------------------------------------------------- night and AutoNight with fov ------------------------------------
@pytest.mark.parametrize("name", ["dog", "horse"])
def test_night_with_fov_against_the_oracle(oracle, name):
    from animal_vision_amd.dichromat import NightSpec

    for geometry in (WR.CAT_GEOMETRY, WR.TWO_EYES):
        animal = _animal(name, geometry, night=NightSpec(bloom=0.12))
        for kind, H, W in [("lamps", 13, 13), ("noise", 37, 70), ("lamps", 96, 131)]:
            frame = N.frames(kind, H, W, seed=5)
            base, out = animal.visualize(frame)
            assert np.array_equal(base, WR.baseline(frame, geometry))
            _check(oracle, name, frame, geometry, out, (name, geometry, kind, H, W, "night"), rod=WR.ROD_DEFAULT, bloom=0.12)


@pytest.mark.parametrize("name", ["dog", "horse"])
def test_auto_night_with_fov_alternating_batch(oracle, name):
    from animal_vision_amd.animals._dichromats import WideStreamOp
    from animal_vision_amd.dichromat import AutoNight, NightSpec

    H, W = 37, 70
    modes = "DNDNND"
    frames = np.stack([DN.scene(m, H, W, i) for i, m in enumerate(modes)])
    assert [DN.oracle_night(f, 0.12) for f in frames] == [m == "N" for m in modes]
    auto = _animal(name, WR.TWO_EYES, night=AutoNight(NightSpec(bloom=0.12), 0.12))
    sop = WideStreamOp(auto, H, W, depth=1, batch=6)
    try:
        d_in, d_out = sop.slot_buffers(0)
        sop.ctx.upload(frames, d_in)
        sop.run_device(d_in, d_out, 6, H, W)
        out = sop.ctx.download(d_out, frames.shape, np.uint8)
        assert sop.last_modes.dtype == np.uint8 and sop.last_modes.tolist() == [int(m == "N") for m in modes]
        assert sop.auto_counts == [3, 6]
    finally:
        sop.close()
    for k, m in enumerate(modes):
        night = m == "N"
        _check(oracle, name, frames[k], WR.TWO_EYES, out[k], (name, k, m), rod=WR.ROD_DEFAULT if night else None, bloom=0.12 if night else 0.0)
        _same(auto.visualize(frames[k])[1], out[k], (name, "visualize", k))


# ---------------------------------------------------------------- Cat -------------------------------------------------------------
def test_cat_with_its_own_constants_as_fov_is_cat(ctx):
    from animal_vision_amd.animals import Cat
    from animal_vision_amd.dichromat import FovSpec

    for H, W in [(6, 5), (37, 53), (96, 160)]:
        frame = _noise(H * W, H, W, 3)
        base, out = Cat().visualize(frame)
        fbase, fout = Cat(fov=FovSpec(105, 40)).visualize(frame)
        _same(fout, out, (H, W, "wide view"))
        _same(fbase, base, (H, W, "baseline"))


def test_cat_with_another_fov_against_the_oracle(oracle):
    from animal_vision_amd.animals import Cat

    phi, overlap, camera = WR.TWO_EYES
    cat = Cat(fov=(phi, overlap, camera))
    for kind, H, W in [("noise", 13, 13), ("ramp", 37, 70), ("noise", 96, 131)]:
        frame = N.frames(kind, H, W, seed=2)
        base, out = cat.visualize(frame)
        assert np.array_equal(base, WR.baseline(frame, WR.TWO_EYES))
        _check(oracle, "cat", frame, WR.TWO_EYES, out, ("cat", kind, H, W))
        assert not np.array_equal(out, Cat().visualize(frame)[1])


def test_cat_descriptor_through_the_new_entry_is_avx_cat_wide(G, ctx):
    """avx_dichromat_wide_u8 with Cat's descriptor: the bytes of avx_cat_wide_u8, which are the chain's (tests/test_cat_stream_gpu.py)."""
    from animal_vision_amd.animals import Cat

    frames = _noise(4, 2, 70, 131, 3)
    want = _chain(G, ctx, frames, Cat.SPEC, WR.CAT_GEOMETRY)
    _same(_entry(G, ctx, frames, Cat.SPEC, WR.CAT_GEOMETRY), want, "cat desc")


# ---------------------------------------------------------------- the stream ------------------------------------------------------
@pytest.fixture(scope="module")
def stream_frames():
    from animal_vision_amd.synthetic import noise_frame, structured_frame

    return [structured_frame(20 + i, 96, 160) if i % 2 else noise_frame(20 + i, 96, 160) for i in range(7)]


def _through_pipeline(op, frames, H, W, **kw):
    from animal_vision_amd.pipeline import FramePipeline

    pipe = FramePipeline(op, H, W, **kw)
    got = {}
    try:
        st = pipe.run(iter(enumerate(frames)), lambda i, o: got.__setitem__(i, o.copy()))
    finally:
        pipe.close()
    assert st.frames == len(frames) and sorted(got) == list(range(len(frames)))
    return [got[i] for i in range(len(frames))]


@pytest.mark.parametrize("io_format", ["rgb", "i420"])
@pytest.mark.parametrize("name", ["dog", "horse"])
def test_stream_equals_visualize_and_split_compose(ctx, stream_frames, name, io_format):
    """7 frames, depth 2, batch 3: two full slots and a partial one, the split frame composed against the zoomed baseline."""
    from animal_vision_amd.animals._dichromats import WideStreamOp
    from animal_vision_amd.renderers import split_compose
    from animal_vision_amd.video import stream_op

    H, W = 96, 160
    animal = _animal(name, WR.TWO_EYES)
    op = stream_op(animal, H, W, 2, 3)
    assert type(op) is WideStreamOp and op.max_batch == 3 and op.slot_baseline(0) is not op.slot_buffers(0)[0]
    try:
        if io_format == "rgb":
            got = _through_pipeline(op, stream_frames, H, W, depth=2, split_compare=True, split_baseline=True, batch=3)
            sources = stream_frames
        else:
            payloads = R.encode(np.stack(stream_frames))
            got = _through_pipeline(op, list(payloads), H, W, depth=2, split_compare=True, split_baseline=True, batch=3, io_format="i420")
            sources = R.decode(payloads, H, W)
    finally:
        op.close()
    for k, f in enumerate(sources):
        base, out = animal.visualize(f)
        assert not np.array_equal(base, f)
        want = split_compose(base, out, left_label="Original", right_label="Transformed")
        _same(got[k], want if io_format == "rgb" else R.encode(want), (name, io_format, k))


def _read_y4m(path):
    from animal_vision_amd.renderers.y4m import Y4MReader

    rd = Y4MReader(path)
    out = []
    while (f := rd.read()) is not None:
        out.append(f)
    rd.close()
    return out


def test_command_y4m_split_compare_batches_agree_with_visualize(tmp_path, capsys, stream_frames):
    from animal_vision_amd.renderers import split_compose
    from animal_vision_amd.video import main, make_animal, parse_args

    H, W = 96, 160
    payloads = R.encode(np.stack(stream_frames))
    src = str(tmp_path / "in.y4m")
    with open(src, "wb") as f:
        f.write(R.y4m_bytes(list(payloads), H, W, header="F25:1 Ip A1:1 C420jpeg XYSCSS=420JPEG"))
    one, three = str(tmp_path / "b1.y4m"), str(tmp_path / "b3.y4m")
    flags = ["--species", "Horse", "--fov", "50:80", "--split-compare"]
    assert main([src, one, *flags]) == 0
    assert "7 frames" in capsys.readouterr().err
    assert main([src, three, *flags, "--batch", "3", "--depth", "2"]) == 0
    assert "7 frames" in capsys.readouterr().err
    assert open(one, "rb").read() == open(three, "rb").read()
    frames = _read_y4m(three)
    assert len(frames) == 7
    horse = make_animal(parse_args([src, three, *flags]))
    for k, rgb in enumerate(R.decode(payloads, H, W)):
        base, out = horse.visualize(rgb)
        assert not np.array_equal(base, rgb)  # the left half is the zoomed baseline, not the input
        _same(frames[k], R.encode(split_compose(base, out, left_label="Original", right_label="Transformed")), k)


def test_command_raw_nv12_scaled(tmp_path, capsys):
    from animal_vision_amd import yuv
    from animal_vision_amd.synthetic import structured_frame
    from animal_vision_amd.video import main

    H, W, Hd, Wd, fmt = 96, 160, 48, 80, "nv12"
    payloads = yuv.rgb_to_yuv(np.stack([structured_frame(70 + i, H, W) for i in range(3)]), pix_fmt=fmt)
    src, dst = str(tmp_path / "in.yuv"), str(tmp_path / "dog.yuv")
    payloads.tofile(src)
    assert main([src, dst, "--species", "Dog", "--fov", "105:40", "--pix-fmt", fmt, "--size", f"{W}x{H}", "--scale", f"{Wd}x{Hd}", "--batch", "2"]) == 0
    assert "3 frames" in capsys.readouterr().err
    got = np.frombuffer(open(dst, "rb").read(), np.uint8).reshape(3, -1)
    assert got.shape[1] == yuv.frame_size(fmt, Hd, Wd)
    small = yuv.yuv_to_rgb_scaled(payloads, H, W, Hd, Wd, pix_fmt=fmt)
    dog = _animal("dog", WR.CAT_GEOMETRY)
    for k in range(3):
        _same(got[k], yuv.rgb_to_yuv(dog.visualize(small[k])[1], pix_fmt=fmt), k)


# ---------------------------------------------------------------- refusals, ordering ----------------------------------------------
def _err(ctx):
    from animal_vision_amd._lib import lib

    return lib.avx_last_error(ctx._h).decode()


def test_entry_refusals(G, ctx):
    from animal_vision_amd._lib import AVX_ERR_INVALID, AVX_OK, AVX_POST_ROWGAIN, AVX_POST_STREAK, DichromatDesc, lib
    from animal_vision_amd.animals import Cat
    from animal_vision_amd.dichromat import DichromatOp

    H, W = 16, 24
    op = DichromatOp(_spec("Dog"), ctx)
    cat_op = DichromatOp(Cat.SPEC, ctx)
    tab, ptrs = G.binocular_warp_tables_device(ctx, _tables(G, H, W, WR.TWO_EYES))
    d_in, d_out = ctx.upload(_noise(0, H, W, 3)), ctx.upload(np.full((H, W, 3), 0x5A, np.uint8))

    def call(inp=d_in.ptr, out=d_out.ptr, n=1, h=H, w=W, desc=op.desc, tables=None, null_desc=False):
        t = list(ptrs if tables is None else tables)
        return lib.avx_dichromat_wide_u8(ctx._h, inp, out, n, h, w, None if null_desc else ctypes.byref(desc), *t, ctx.stream)

    def desc_with(base=op.desc, **kw):
        d = DichromatDesc.from_buffer_copy(bytes(base))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    try:
        bad = [dict(inp=None), dict(out=None), dict(out=d_in.ptr), dict(n=-1), dict(h=0), dict(w=0), dict(h=-3), dict(null_desc=True),
               dict(desc=desc_with(struct_size=ctypes.sizeof(DichromatDesc) - 4)), dict(desc=desc_with(color_mode=2)), dict(desc=desc_with(post_mode=7)),
               dict(desc=desc_with(post_mode=-1)), dict(desc=desc_with(ksize=0)), dict(desc=desc_with(ksize=8)), dict(desc=desc_with(ksize=35)),
               dict(desc=desc_with(ksize=-9)), dict(desc=desc_with(post_mode=AVX_POST_ROWGAIN)),  # no row gains
               dict(desc=desc_with(post_mode=AVX_POST_STREAK)),  # no row tables
               dict(desc=desc_with(cat_op.desc, post_mode=AVX_POST_STREAK))]  # the streak blur runs on the matrix colour stage
        bad += [dict(tables=[None if j == i else p for j, p in enumerate(ptrs)]) for i in range(5)]
        for kw in bad:
            assert call(**kw) == AVX_ERR_INVALID, kw
            assert _err(ctx).startswith("avx_dichromat_wide_u8:"), (kw, _err(ctx))
        assert call(n=0) == AVX_OK
        ctx.sync()
        assert (ctx.download(d_out, (H, W, 3), np.uint8) == 0x5A).all()  # no refused call, nor n_frames == 0, wrote anything
        assert call(desc=desc_with(in_f32=1, variant=2)) == AVX_OK  # both ignored
        got = ctx.download(d_out, (H, W, 3), np.uint8)
        assert call() == AVX_OK
        assert np.array_equal(got, ctx.download(d_out, (H, W, 3), np.uint8))
    finally:
        d_in.free(); d_out.free(); tab.free()


@pytest.mark.parametrize("route", ROUTES)
def test_two_calls_on_one_stream_without_synchronisation(G, ctx, monkeypatch, route):
    """The second call reuses the stream workspace's flags and scratch: stream order alone must keep the two apart."""
    from animal_vision_amd.dichromat import DichromatOp

    monkeypatch.setenv("AVX_WIDE_ROUTE", route)
    H, W = 70, 131
    a, b = _noise(31, 2, H, W, 3), _noise(32, 2, H, W, 3)
    b[0] &= 1
    spec = _spec("Raccoon")
    want_a, want_b = _entry(G, ctx, a, spec, WR.TWO_EYES), _entry(G, ctx, b, spec, WR.TWO_EYES)  # each followed by a synchronising download
    op = DichromatOp(spec, ctx)
    tab, ptrs = G.binocular_warp_tables_device(ctx, _tables(G, H, W, WR.TWO_EYES))
    d_a, d_b = ctx.upload(a), ctx.upload(b)
    o_a, o_b = ctx.malloc(a.nbytes), ctx.malloc(b.nbytes)
    try:
        G.dichromat_wide_device(ctx, d_a, o_a, 2, H, W, op.desc, ptrs)
        G.dichromat_wide_device(ctx, d_b, o_b, 2, H, W, op.desc, ptrs)
        _same(ctx.download(o_a, a.shape, np.uint8), want_a, "first call")
        _same(ctx.download(o_b, b.shape, np.uint8), want_b, "second call")
    finally:
        for buf in (d_a, d_b, o_a, o_b, tab):
            buf.free()
