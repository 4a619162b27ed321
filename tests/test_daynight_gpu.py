"""GPU: the per-frame day/night switch (csrc/daynight.hip).

The decision: dichromat.luma_modes against oracle.np_backend.NumpyProbes.median_luma(frame) < T, and the three fields of every
record against NumPy on the oracle's Y -- integers and float32 bit patterns.  The routing: every frame of a switched batch byte for
byte what the day entry or the night entry writes for that frame alone.  No tolerance anywhere."""
import numpy as np
import pytest

import _daynight_ref as R

pytestmark = pytest.mark.gpu


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _check_records(frames, T, got, what):
    night, below, a, b = got
    assert night.dtype == np.bool_ and below.dtype == np.uint32 and a.dtype == np.float32 and b.dtype == np.float32
    for k, f in enumerate(frames):
        c, lo, hi = R.record(f, T)
        assert int(below[k]) == c, (what, k, int(below[k]), c)
        assert _bits(a[k]) == _bits(lo) and _bits(b[k]) == _bits(hi), (what, k, float(a[k]), float(lo), float(b[k]), float(hi))
        assert bool(night[k]) is R.oracle_night(f, T), (what, k)


# ---------------------------------------------------------------- the decision ----------------------------------------------------
@pytest.mark.parametrize("H,W", R.SIZES)
def test_records_and_decisions_against_numpy(H, W):
    """Every kind of frame at every threshold, as one mixed batch (13 frames) and frame by frame: the same bytes."""
    from animal_vision_amd.dichromat import luma_modes

    frames = np.stack([R.frame(k, H, W) for k in R.KINDS])
    for T in R.THRESHOLDS:
        batch = luma_modes(frames, T)
        _check_records(frames, T, batch, (H, W, T))
        for k, f in enumerate(frames):
            single = luma_modes(f, T)
            for x, y in zip(batch, single):
                assert x[k:k + 1].tobytes() == y.tobytes(), (H, W, T, R.KINDS[k])
    if H * W % 2 == 0:  # the straddle is reached, and decided by the two kept values
        night, below, _, _ = luma_modes(frames, 0.12)
        i, j = R.KINDS.index("half30_31"), R.KINDS.index("half30_32")
        assert below[i] * 2 == H * W == below[j] * 2 and night[i] and not night[j]
    assert not luma_modes(frames, 0.0)[0].any()  # never night


@pytest.mark.parametrize("H,W", [(3, 5), (37, 70), (64, 48)])
def test_batches_of_1_3_and_16_give_each_frame_its_single_record(H, W):
    from animal_vision_amd.dichromat import luma_modes

    kinds = (R.KINDS + ["colour", "noise", "half30_31"])[:16]
    frames = np.stack([R.frame(k, H, W, seed=i) for i, k in enumerate(kinds)])
    single = [luma_modes(f, 0.12) for f in frames]
    modes = [bool(s[0][0]) for s in single]
    assert True in modes and False in modes  # mixed
    for n in (1, 3, 16):
        for f0 in range(0, 16 - n + 1, 5):
            got = luma_modes(frames[f0:f0 + n], 0.12)
            for k in range(n):
                for x, y in zip(got, single[f0 + k]):
                    assert x[k:k + 1].tobytes() == y.tobytes(), (H, W, n, f0, k)
    got = luma_modes(np.concatenate([frames, frames[:3]]), 0.12)  # more than one call's worth
    assert got[0].shape == (19,) and np.array_equal(got[1][16:], got[1][:3])


def test_a_frame_one_byte_into_its_buffer_takes_the_byte_path():
    """64 x 48 is a multiple of 16 pixels, but at an odd address nothing is read 16 bytes at a time: the same record."""
    from animal_vision_amd import _lib
    from animal_vision_amd.dichromat import finish_modes, luma_modes, luma_records_device
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 64, 48
    for kind in ("colour", "noise", "half30_31", "last_below"):
        frames = np.stack([R.frame(kind, H, W, seed=s) for s in (0, 1)])
        host = np.zeros(frames.nbytes + 16, np.uint8)
        host[1:1 + frames.nbytes] = frames.reshape(-1)
        d_in, d_rec = ctx.upload(host), ctx.malloc(16 * 16)
        try:
            assert d_in.ptr % 16 == 0
            rec = luma_records_device(ctx, d_in.ptr + 1, 2, H, W, 0.12, d_rec).copy()
        finally:
            d_in.free()
            d_rec.free()
        assert rec.dtype == np.dtype(_lib.LUMA_MODE_REC_DTYPE)
        night = finish_modes(rec["below"], rec["max_below"], rec["min_at_or_above"], H * W, 0.12)
        _check_records(frames, 0.12, (night, rec["below"], rec["max_below"], rec["min_at_or_above"]), kind)
        want = luma_modes(frames, 0.12)
        assert rec["below"].tobytes() == want[1].tobytes() and rec["max_below"].tobytes() == want[2].tobytes()
        assert rec["min_at_or_above"].tobytes() == want[3].tobytes()


def test_the_decision_entry_refuses_by_name():
    from animal_vision_amd._lib import AvxError
    from animal_vision_amd.dichromat import luma_records_device
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    d_in, d_rec = ctx.malloc(17 * 48), ctx.malloc(17 * 16)
    try:
        for n, H, W, T, rec_off, word in ((0, 4, 4, 0.12, 0, "n_frames"), (17, 4, 4, 0.12, 0, "n_frames"), (1, 0, 4, 0.12, 0, "frame size"),
                                          (1, 4, 4, 1.5, 0, "threshold"), (1, 4, 4, 0.12, 4, "aligned")):
            with pytest.raises(AvxError) as e:
                luma_records_device(ctx, d_in.ptr, n, H, W, T, d_rec.view(rec_off, 16 * 16))
            assert "avx_luma_mode_u8:" in str(e.value) and word in str(e.value), str(e.value)
    finally:
        d_in.free()
        d_rec.free()


# ---------------------------------------------------------------- the routing -----------------------------------------------------
def _spec(name):
    from animal_vision_amd import animals

    return getattr(animals, name).SPEC


@pytest.mark.parametrize("H,W", [(13, 13), (37, 70), (96, 131)])
@pytest.mark.parametrize("name", ["Dog", "Lion", "Sheep", "Rat", "Pig", "Cat"])
def test_switched_batches_are_the_day_and_night_entries_frame_by_frame(name, H, W):
    from animal_vision_amd.dichromat import AutoNight, DichromatOp, NightSpec

    days = [R.scene("D", H, W, s) for s in range(5)]
    nights = [R.scene("N", H, W, s) for s in range(5)]
    for f in days:
        assert not R.oracle_night(f, 0.12)
    for f in nights:
        assert R.oracle_night(f, 0.12)
    spec = _spec(name)
    day_op = DichromatOp(spec)
    day_out = [day_op(f) for f in days]
    for bloom in (0.0, 0.12):
        night_op = DichromatOp(spec, night=NightSpec(bloom=bloom))
        night_out = [night_op(f) for f in nights]
        auto = DichromatOp(spec, night=AutoNight(NightSpec(bloom=bloom), 0.12))
        mixed = [("D", 0), ("N", 0), ("N", 1), ("D", 1), ("N", 2)]
        for plan in (mixed, [("D", k) for k in range(5)], [("N", k) for k in range(5)]):
            batch = np.stack([(days if m == "D" else nights)[k] for m, k in plan])
            got = auto(batch)
            assert auto.last_modes.dtype == np.uint8
            assert auto.last_modes.tolist() == [int(R.oracle_night(f, 0.12)) for f in batch] == [int(m == "N") for m, _ in plan]
            for i, (m, k) in enumerate(plan):
                want = day_out[k] if m == "D" else night_out[k]
                assert np.array_equal(got[i], want), (name, H, W, bloom, i, m)
        assert not np.array_equal(night_out[0], day_op(nights[0]))  # the two routes are told apart by their bytes
    assert auto.auto_counts == [8, 15]
    # a threshold that turns every frame: 0 is never night, 1 is night for all of these
    batch = np.stack([days[0], nights[0]])
    assert np.array_equal(DichromatOp(spec, night=AutoNight(threshold=0.0))(batch), np.stack([day_op(days[0]), day_op(nights[0])]))
    always = DichromatOp(spec, night=AutoNight(threshold=1.0))
    always(batch)
    assert always.last_modes.tolist() == [1, 1]


def test_visualize_with_auto_night_is_the_day_or_the_night_result():
    from animal_vision_amd.animals import Cat, Dog, Sheep
    from animal_vision_amd.dichromat import AutoNight, NightSpec

    H, W = 37, 70
    for cls in (Dog, Sheep, Cat):
        auto, day, night = cls(night=AutoNight(NightSpec(bloom=0.12))), cls(), cls(night=NightSpec(bloom=0.12))
        for mode, ref in (("D", day), ("N", night)):
            f = R.scene(mode, H, W, 7)
            base, out = auto.visualize(f)
            want_base, want = ref.visualize(f)
            assert np.array_equal(out, want) and np.array_equal(base, want_base), (cls.__name__, mode)
            if cls is not Cat:
                assert base is f


# ---------------------------------------------------------------- Cat's stream operator, the frame pipeline ------------------------
def _clip(H, W):
    """12 frames that cross the threshold twice: day, dusk, night, dawn."""
    modes = "DDDNNNNDDDNN"
    frames = [R.scene(m, H, W, i) for i, m in enumerate(modes)]
    assert [R.oracle_night(f, 0.12) for f in frames] == [m == "N" for m in modes] and modes.count("N") == 6
    return modes, frames


def _run(pipe, frames):
    got = {}
    pipe.run(((i, f) for i, f in enumerate(frames)), lambda i, o: got.__setitem__(i, o))
    pipe.close()
    return [got[i] for i in range(len(frames))]


@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("warp", [True, False])
def test_cat_stream_op_and_frame_pipeline_against_visualize(batch, warp):
    from animal_vision_amd.animals import Cat
    from animal_vision_amd.animals._dichromats import CatStreamOp
    from animal_vision_amd.dichromat import AutoNight, NightSpec
    from animal_vision_amd.pipeline import FramePipeline

    H, W = 64, 96
    modes, frames = _clip(H, W)
    cls = Cat if warp else type("CatNoWarp", (Cat,), {"ENABLE_FOV_WARP": False})
    auto, day, night = cls(night=AutoNight(NightSpec(bloom=0.12))), cls(), cls(night=NightSpec(bloom=0.12))
    want = [(night if m == "N" else day).visualize(f)[1] for m, f in zip(modes, frames)]
    assert not np.array_equal(want[3], day.visualize(frames[3])[1])
    for k, f in enumerate(frames):  # visualize() itself: one frame through the stream operator
        assert np.array_equal(auto.visualize(f)[1], want[k]), k
    sop = CatStreamOp(auto, H, W, depth=2, batch=batch)
    try:
        got = _run(FramePipeline(sop, H, W, depth=2, batch=batch), frames)
        assert sop.auto_counts == [modes.count("N"), 12]
    finally:
        sop.close()
    for k in range(12):
        assert np.array_equal(got[k], want[k]), (batch, warp, k, modes[k])


@pytest.mark.parametrize("batch", [1, 4])
def test_frame_pipeline_with_a_dichromat_op(batch):
    from animal_vision_amd.animals import Rat
    from animal_vision_amd.dichromat import AutoNight, DichromatOp, NightSpec
    from animal_vision_amd.pipeline import FramePipeline

    H, W = 37, 70
    modes, frames = _clip(H, W)
    day, night = DichromatOp(Rat.SPEC), DichromatOp(Rat.SPEC, night=NightSpec())
    op = DichromatOp(Rat.SPEC, night=AutoNight())
    got = _run(FramePipeline(op, H, W, depth=2, batch=batch), frames)
    for k, (m, f) in enumerate(zip(modes, frames)):
        assert np.array_equal(got[k], (night if m == "N" else day)(f)), (batch, k)
    assert op.auto_counts == [6, 12]


# ---------------------------------------------------------------- the video command -----------------------------------------------
@pytest.mark.parametrize("species,extra", [("Dog", ["--bloom", "0.12", "--batch", "4", "--depth", "2"]), ("Cat", ["--batch", "1"])])
def test_video_command_switches_per_frame(tmp_path, capsys, species, extra):
    from animal_vision_amd.video import main, make_animal, parse_args

    H, W = 64, 96
    modes, frames = _clip(H, W)
    src, dst = str(tmp_path / "clip.npy"), str(tmp_path / "out.npy")
    np.save(src, np.stack(frames))
    argv = [src, dst, "--species", species, "--night-auto"] + extra
    assert main(argv) == 0
    err = capsys.readouterr().err
    assert "12 frames" in err and "night-auto: 6 of 12 frames night (threshold 0.12)" in err, err
    got = np.load(dst)
    assert got.shape == (12, H, W, 3)
    bloom = ["--bloom", "0.12"] if "--bloom" in extra else []
    day = make_animal(parse_args([src, dst, "--species", species]))
    night = make_animal(parse_args([src, dst, "--species", species, "--night"] + bloom))
    for k, (m, f) in enumerate(zip(modes, frames)):
        assert np.array_equal(got[k], (night if m == "N" else day).visualize(f)[1]), (species, k, m)
    # a threshold of 0 is never night: the day command's bytes, and the summary says so
    assert main([src, dst, "--species", species, "--night-auto", "--night-threshold", "0"]) == 0
    assert "night-auto: 0 of 12 frames night (threshold 0)" in capsys.readouterr().err
    for k, f in enumerate(frames):
        assert np.array_equal(np.load(dst)[k], day.visualize(f)[1]), k


# ---------------------------------------------------------------- refusals --------------------------------------------------------
def test_small_frames_are_refused_even_by_day():
    from animal_vision_amd._lib import AvxError
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import AutoNight

    dog = Dog(night=AutoNight())
    for shape in ((12, 40, 3), (40, 12, 3)):
        with pytest.raises(AvxError) as e:
            dog.visualize(np.full(shape, 255, np.uint8))  # a day frame
        assert "avx_dichromat_auto_u8:" in str(e.value) and "smaller than 13 x 13" in str(e.value), str(e.value)
    dog.visualize(np.full((13, 40, 3), 255, np.uint8))


def test_float_input_is_refused_by_name():
    from animal_vision_amd._lib import AvxError
    from animal_vision_amd.animals import Dog
    from animal_vision_amd.dichromat import AutoNight, DichromatOp
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    op = DichromatOp(Dog.SPEC, ctx, night=AutoNight())
    op.desc.in_f32 = 1
    d_in, d_out = ctx.malloc(16 * 16 * 12), ctx.malloc(16 * 16 * 3)
    try:
        with pytest.raises(AvxError) as e:
            op.run_device(d_in, d_out, 1, 16, 16)
        assert "avx_dichromat_auto_u8:" in str(e.value) and "in_f32" in str(e.value), str(e.value)
    finally:
        d_in.free()
        d_out.free()
    with pytest.raises(AvxError) as e:
        DichromatOp(Dog.SPEC, ctx, night=AutoNight()).run_device(ctx.malloc(17 * 16 * 16 * 3), ctx.malloc(17 * 16 * 16 * 3), 17, 16, 16)
    assert "n_frames must be 1..16" in str(e.value)
