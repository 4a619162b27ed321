"""GPU: the dichromats at night (csrc/night.hip) against the oracle composition of tests/_night_ref.py.

Contract: the float pipelines' -- codes within +-1 of the oracle's, with tests/_sensitivity.check_codes' caps at their defaults (at
most 5 % of samples differing, at most 0.2 % beyond +-1, and those only where the jittered oracle itself moves).  Not bit-exact: the
device's powf and Cat's float64 tail, which the device rounds to float32 planes.

Sizes: 13 x 13 (the smallest allowed: every tile is all border, both reflections meet), 37 x 70 (no multiple of a tile, a vector or
4), 96 x 131 (several 64 x 32 tiles each way, odd width), 270 x 480 once."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _night_ref as N
from _sensitivity import check_codes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIES = ["dog", "cat", "sheep", "pig", "cow", "goat", "horse", "rabbit", "panda", "deer", "kangaroo", "rat", "squirrel", "elephant", "lion",
           "tiger", "bear", "wolf", "fox", "raccoon"]
BLOOM_SPECIES = ["dog", "sheep", "rat", "rabbit", "cat"]


def _species(name, night=True, warp=True):
    from animal_vision_amd import animals

    cls = getattr(animals, name.capitalize())
    if name == "cat" and not warp:
        cls = type("CatNoWarp", (cls,), {"ENABLE_FOV_WARP": False})
    return cls(night=night) if night is not None else cls()


def _night(bloom=0.0):
    from animal_vision_amd.dichromat import NightSpec

    return NightSpec(bloom=bloom)


def _check(oracle, name, frame, got, what, bloom=0.0, warp=True):
    sp = oracle.DICHROMATS[name]
    want = N.night_ref(sp, frame, bloom=bloom, cat_warp=warp)
    return check_codes(got, want, what, lambda seed: N.night_ref(sp, frame, bloom=bloom, cat_warp=warp, jit=oracle.relative_jitter(seed)))


# ---------------------------------------------------------------- all 20 species, defaults ----------------------------------------
DEFAULT_CASES = [("noise", 13, 13), ("white", 13, 13), ("ramp", 37, 70), ("dark", 37, 70), ("ones", 37, 70), ("lamps", 96, 131), ("noise", 96, 131),
                 ("black", 37, 70)]


@pytest.mark.parametrize("name", SPECIES)
def test_defaults_against_the_oracle(oracle, name):
    animal = _species(name)
    assert len(oracle.DICHROMATS) == 20 and name in oracle.DICHROMATS
    for kind, H, W in DEFAULT_CASES:
        frame = N.frames(kind, H, W, seed=len(name))
        base, out = animal.visualize(frame)
        assert out.dtype == np.uint8 and out.shape == frame.shape
        if name == "cat":
            assert np.array_equal(base, N.cat_baseline(frame)), (kind, H, W)
        else:
            assert base is frame
        _check(oracle, name, frame, out, (name, kind, H, W))
        if kind == "black":
            assert not out.any()
        if kind == "ones":  # bytes of 1 are 1.0 here, not 1 / 255 (which the rod stage lifts to code 17 at the most): the frame is bright
            assert out.max() > 64, (name, int(out.max()))


def test_cat_without_the_warp_and_its_baseline(oracle):
    cat_day, warp_night, flat_night = _species("cat", night=None), _species("cat"), _species("cat", warp=False)
    for kind, H, W in DEFAULT_CASES:
        frame = N.frames(kind, H, W, seed=3)
        base, out = flat_night.visualize(frame)
        _check(oracle, "cat", frame, out, ("cat, no warp", kind, H, W), warp=False)
        day_base, day_out = cat_day.visualize(frame)
        assert np.array_equal(base, day_base) and np.array_equal(warp_night.visualize(frame)[0], day_base), (kind, H, W)
        if kind in ("noise", "lamps"):
            assert not np.array_equal(out, day_out)  # the night view is not the day view


def test_one_video_sized_frame(oracle):
    frame = N.frames("lamps", 270, 480)
    _, out = _species("lion", night=_night(0.12)).visualize(frame)
    _check(oracle, "lion", frame, out, "lion 270 x 480, bloom 0.12", bloom=0.12)
    # 72 tiles, on every XCD: the all-0/1 frame's second pass must land after every first-pass store, whichever workgroup runs it
    ones = N.frames("ones", 270, 480)
    _, out = _species("dog").visualize(ones)
    assert out.max() > 64
    _check(oracle, "dog", ones, out, "dog 270 x 480, every byte 0 or 1")


def test_other_rod_parameters(oracle):
    from animal_vision_amd.dichromat import NightSpec

    frame = N.frames("noise", 37, 70)
    rod = (0.25, 1.1, 1.3)
    sp = oracle.DICHROMATS["wolf"]
    _, out = _species("wolf", night=NightSpec(*rod, bloom=0.2)).visualize(frame)
    want = N.night_ref(sp, frame, rod=rod, bloom=0.2)
    check_codes(out, want, "wolf, other rod parameters", lambda seed: N.night_ref(sp, frame, rod=rod, bloom=0.2, jit=oracle.relative_jitter(seed)))


# ---------------------------------------------------------------- bloom -----------------------------------------------------------
@pytest.mark.parametrize("name", BLOOM_SPECIES)
@pytest.mark.parametrize("bloom", [0.12, 0.3])
def test_bloom_against_the_oracle(oracle, name, bloom):
    animal = _species(name, night=_night(bloom))
    plain = _species(name)
    moved = 0
    for kind, H, W in [("lamps", 13, 13), ("lamps", 37, 70), ("noise", 37, 70), ("white", 37, 70), ("lamps", 96, 131), ("noise", 96, 131)]:
        frame = N.frames(kind, H, W, seed=7)
        _, out = animal.visualize(frame)
        _check(oracle, name, frame, out, (name, bloom, kind, H, W), bloom=bloom)
        moved = max(moved, int(np.abs(out.astype(int) - plain.visualize(frame)[1].astype(int)).max()))
    assert moved >= 4, (name, bloom, moved)  # the bloom is there: a missing one would still pass a frame it does not change
    for kind in ("black", "dark"):  # the mask is exactly 0: the bytes with bloom are the bytes without it
        frame = N.frames(kind, 37, 70, seed=7)
        assert np.array_equal(animal.visualize(frame)[1], plain.visualize(frame)[1]), (name, bloom, kind)


# ---------------------------------------------------------------- batches ---------------------------------------------------------
def _batch_frames(n, H, W):
    kinds = ["noise", "ones", "lamps", "dark", "black", "ramp", "white"]
    return np.stack([N.frames(kinds[i % len(kinds)], H, W, seed=i) for i in range(n)])


@pytest.mark.parametrize("name,bloom", [("dog", 0.12), ("sheep", 0.0), ("rat", 0.3), ("rabbit", 0.12), ("cat", 0.0)])
def test_batches_equal_single_frames(name, bloom):
    from animal_vision_amd.dichromat import DichromatOp

    H, W = 37, 70
    animal = _species(name, night=_night(bloom), warp=False)
    op = DichromatOp(animal.SPEC, night=animal.night)
    frames = _batch_frames(16, H, W)
    single = np.stack([op(f) for f in frames])
    assert np.array_equal(single[1], animal.visualize(frames[1])[1])
    for n in (1, 3, 16):
        assert np.array_equal(op(frames[:n]), single[:n]), (name, n)
    assert np.array_equal(op(frames[5:8]), single[5:8]), name  # the same frames at other places of a batch


def test_cat_stream_op_batches_with_the_warp():
    from animal_vision_amd.animals._dichromats import CatStreamOp

    H, W = 37, 70
    cat = _species("cat", night=_night(0.12))
    frames = _batch_frames(3, H, W)
    single = [cat.visualize(f) for f in frames]
    sop = CatStreamOp(cat, H, W, depth=1, batch=3)
    try:
        d_in, d_out = sop.slot_buffers(0)
        sop.ctx.upload(frames, d_in)
        sop.run_device(d_in, d_out, 3, H, W)
        out = sop.ctx.download(d_out, frames.shape, np.uint8)
        base = sop.ctx.download(sop.slot_baseline(0), frames.shape, np.uint8)
    finally:
        sop.close()
    for k in range(3):
        assert np.array_equal(out[k], single[k][1]) and np.array_equal(base[k], single[k][0]), k


_GROUP_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import _night_ref as N
from animal_vision_amd.animals import Dog, Rabbit
from animal_vision_amd.dichromat import DichromatOp, NightSpec
kinds = ["noise", "ones", "lamps", "dark", "ramp"]
frames = np.stack([N.frames(k, 37, 70, seed=i) for i, k in enumerate(kinds)])
for cls in (Dog, Rabbit):
    op = DichromatOp(cls.SPEC, night=NightSpec(bloom=0.12))
    np.save({out!r} + cls.__name__ + ".npy", op(frames))
print("walked")
"""


def test_group_walk_in_a_fresh_process(tmp_path):
    """A batch of 5 in groups of 2 (AVX_NIGHT_GROUP, read per call by the library; set for a child so that no other test sees it)."""
    from animal_vision_amd.animals import Dog, Rabbit
    from animal_vision_amd.dichromat import DichromatOp

    out = str(tmp_path / "group_")
    env = dict(os.environ, AVX_NIGHT_GROUP="2")
    script = _GROUP_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "walked" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    kinds = ["noise", "ones", "lamps", "dark", "ramp"]
    frames = [N.frames(k, 37, 70, seed=i) for i, k in enumerate(kinds)]
    for cls in (Dog, Rabbit):
        op = DichromatOp(cls.SPEC, night=_night(0.12))
        got = np.load(out + cls.__name__ + ".npy")
        for k, f in enumerate(frames):
            assert np.array_equal(got[k], op(f)), (cls.__name__, k)


# ---------------------------------------------------------------- refusals --------------------------------------------------------
def test_small_frames_are_refused_by_name():
    from animal_vision_amd._lib import AvxError

    for shape in ((12, 40, 3), (40, 12, 3)):
        with pytest.raises(AvxError) as e:
            _species("dog").visualize(np.zeros(shape, np.uint8))
        assert "avx_dichromat_night_u8:" in str(e.value) and "smaller than 13 x 13" in str(e.value), str(e.value)
    _species("dog").visualize(np.zeros((13, 40, 3), np.uint8))


@pytest.mark.parametrize("name", ["dog", "sheep", "cat"])
def test_float_frames_are_not_implemented_at_night(name):
    for dt in (np.float32, np.float64):
        with pytest.raises(NotImplementedError) as e:
            _species(name).visualize(np.zeros((16, 16, 3), dt))
        assert "night" in str(e.value)


# ---------------------------------------------------------------- the video command -----------------------------------------------
def _source_frames(spec):
    from animal_vision_amd.renderers import VideoRenderer

    src = VideoRenderer(read_path=spec)
    src.open()
    out = []
    while True:
        f = src.get_image()
        if f is None:
            src.close()
            return out
        out.append(f)


@pytest.mark.parametrize("species,extra", [("Dog", ["--bloom", "0.12"]), ("Cat", [])])
def test_video_command_streams_the_night_view(tmp_path, capsys, species, extra):
    from animal_vision_amd.video import main, make_animal, parse_args

    src, dst = "synthetic:96x64:5:structured", str(tmp_path / "night.npy")
    argv = ["--species", species, "--night"] + extra
    frames = _source_frames(src)
    assert len(frames) == 5 and frames[0].shape == (64, 96, 3)
    animal = make_animal(parse_args([src, dst] + argv))
    assert animal.night is not None and animal.night.bloom == (0.12 if extra else 0.0)
    assert main([src, dst] + argv + ["--batch", "2", "--split-compare", "--no-labels"]) == 0
    assert "5 frames" in capsys.readouterr().err
    got = np.load(dst)
    assert got.shape == (5, 64, 96, 3)
    day = make_animal(parse_args([src, dst, "--species", species]))
    for k, f in enumerate(frames):
        base, out = animal.visualize(f)
        assert np.array_equal(got[k][:, 49:], out[:, 49:]), k   # right of the 1-px seam at W // 2: visualize()'s bytes
        assert np.array_equal(got[k][:, :48], base[:, :48]), k  # left of it: the baseline -- the input, or Cat's zoomed view
        if species == "Dog":
            assert base is f
        assert not np.array_equal(out, day.visualize(f)[1]), k
