"""CPU: the per-frame day/night switch as far as it can be checked without a GPU -- the finishing rule of the one-pass
decision (in Python and in the library) against np.median, the luma tables, AutoNight's validation, the `video` command's
--night-auto / --night-threshold, the struct and the declarations and exports of the entry points."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import _daynight_ref as R
from conftest import GOLDEN


def _records(frames, T):
    rec = [R.record(f, T) for f in frames]
    return (np.array([r[0] for r in rec], np.uint32), np.array([r[1] for r in rec], np.float32), np.array([r[2] for r in rec], np.float32))


def _library_modes(below, max_below, min_at, H, W, T):
    from animal_vision_amd import _lib

    rec = np.zeros(below.size, _lib.LUMA_MODE_REC_DTYPE)
    rec["below"], rec["max_below"], rec["min_at_or_above"] = below, max_below, min_at
    modes = np.full(below.size, 7, np.uint8)
    assert _lib.lib.avx_luma_mode_finish(None, rec.ctypes.data, below.size, H, W, float(T), modes.ctypes.data) == _lib.AVX_OK
    return modes


@pytest.mark.parametrize("H,W", [s for s in R.SIZES if s != (270, 480)])
def test_finishing_rule_is_the_median(H, W):
    """Records formed by NumPy from the oracle's Y: the rule gives float(np.median(Y)) < T, in Python and in the library."""
    from animal_vision_amd.dichromat import finish_modes

    frames = [R.frame(k, H, W, seed=s) for k in R.KINDS for s in (0, 1)][:16 * 2]
    for T in R.THRESHOLDS + [0.1196, 0.1235]:
        want = np.array([R.oracle_night(f, T) for f in frames])
        assert np.array_equal(want, np.array([float(np.median(R.luma(f))) < T for f in frames]))
        below, a, b = _records(frames, T)
        assert np.array_equal(finish_modes(below, a, b, H * W, T), want), (H, W, T)
        for f0 in range(0, len(frames), 16):
            got = _library_modes(below[f0:f0 + 16], a[f0:f0 + 16], b[f0:f0 + 16], H, W, T)
            assert np.array_equal(got, want[f0:f0 + 16].astype(np.uint8)), (H, W, T, f0)


def test_the_straddle_cases_are_reached():
    """Even n with below == n / 2: the count alone cannot decide, the two kept values do -- night with 30 | 31, day with 30 | 32."""
    from animal_vision_amd.dichromat import finish_modes

    for H, W in ((1, 2), (2, 2), (64, 48), (37, 70)):
        n = H * W
        for kind, night in (("half30_31", True), ("half30_32", False)):
            f = R.frame(kind, H, W)
            below, a, b = R.record(f, 0.12)
            assert below * 2 == n and a < 0.12 <= b
            assert bool(finish_modes([below], [a], [b], n, 0.12)[0]) is night is R.oracle_night(f, 0.12), (H, W, kind)
        for kind, c in (("half30_31_more", n // 2 + 1), ("half30_31_less", n // 2 - 1), ("half30_32_more", n // 2 + 1)):
            f = R.frame(kind, H, W)
            assert R.record(f, 0.12)[0] == c
            assert bool(finish_modes(*[[v] for v in R.record(f, 0.12)], n, 0.12)[0]) is (2 * c > n) is R.oracle_night(f, 0.12)
    assert abs(float(R.luma(R.frame("grey30", 1, 1))[0, 0]) - 0.1176) < 1e-4 and abs(float(R.luma(R.frame("grey31", 1, 1))[0, 0]) - 0.1216) < 1e-4


def test_luma_tables_are_numpys_and_the_librarys():
    from animal_vision_amd.dichromat import luma_tables
    from animal_vision_amd.runtime import get_table

    t = luma_tables()
    assert t.shape == (3, 256) and t.dtype == np.float32
    x = np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0
    for c, w in enumerate((0.2126, 0.7152, 0.0722)):
        assert np.array_equal(t[c].view(np.uint32), (w * x).view(np.uint32))
    lib_t = get_table(3)
    assert lib_t.dtype == np.float32 and lib_t.size == 768
    assert np.array_equal(lib_t.view(np.uint32), t.reshape(-1).view(np.uint32))  # what the kernel adds up
    f = R.frame("colour", 37, 70)
    Y = (t[0][f[..., 0]] + t[1][f[..., 1]]) + t[2][f[..., 2]]
    assert np.array_equal(Y.view(np.uint32), R.luma(f).view(np.uint32))  # two float32 adds per pixel give the oracle's Y
    assert float(Y.min()) >= 0.0  # the order of the bit patterns is the order of the values


def test_finish_refuses_bad_arguments():
    from animal_vision_amd import _lib

    rec = np.zeros(2, _lib.LUMA_MODE_REC_DTYPE)
    modes = np.zeros(2, np.uint8)
    fin = _lib.lib.avx_luma_mode_finish
    assert fin(None, rec.ctypes.data, 2, 4, 4, 0.12, modes.ctypes.data) == _lib.AVX_OK
    for args in ((None, 2, 4, 4, 0.12, modes.ctypes.data), (rec.ctypes.data, 2, 4, 4, 0.12, None), (rec.ctypes.data, 0, 4, 4, 0.12, modes.ctypes.data),
                 (rec.ctypes.data, 17, 4, 4, 0.12, modes.ctypes.data), (rec.ctypes.data, 2, 0, 4, 0.12, modes.ctypes.data),
                 (rec.ctypes.data, 2, 4, 4, 1.5, modes.ctypes.data), (rec.ctypes.data, 2, 4, 4, float("nan"), modes.ctypes.data)):
        assert fin(None, *args) == _lib.AVX_ERR_INVALID, args
    rec["below"][1] = 17  # more than 4 x 4 pixels
    assert fin(None, rec.ctypes.data, 2, 4, 4, 0.12, modes.ctypes.data) == _lib.AVX_ERR_INVALID


def test_auto_night_defaults_and_validation():
    from animal_vision_amd.animals import Cat, Dog
    from animal_vision_amd.dichromat import AutoNight, DichromatOp, NightSpec

    a = AutoNight()
    assert a.night == NightSpec() and a.threshold == 0.12
    assert AutoNight(NightSpec(bloom=0.3), 0.0).threshold == 0.0 and AutoNight(threshold=1).threshold == 1
    assert hash(AutoNight()) == hash(AutoNight(NightSpec(), 0.12)) and AutoNight() != AutoNight(threshold=0.2)
    with pytest.raises(Exception):
        a.threshold = 0.5  # frozen
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "0.12", True, None):
        with pytest.raises(ValueError) as e:
            AutoNight(threshold=bad)
        assert "threshold" in str(e.value), bad
    for bad in (True, None, 0.12, "night"):
        with pytest.raises(TypeError):
            AutoNight(night=bad)
    # accepted wherever night= is; True and a NightSpec keep their meaning
    op = DichromatOp(Dog.SPEC, night=AutoNight(NightSpec(bloom=0.12), 0.2))
    assert op.auto == AutoNight(NightSpec(bloom=0.12), 0.2) and op.night is op.auto and op.night_desc.bloom_strength == 0.12 and op.max_batch == 16
    assert op.last_modes.dtype == np.uint8 and op.last_modes.size == 0
    plain = DichromatOp(Dog.SPEC, night=NightSpec())
    assert plain.auto is None and plain.night == NightSpec() and DichromatOp(Dog.SPEC).auto is None
    dog, cat = Dog(night=AutoNight()), Cat(night=AutoNight(threshold=0.3))
    assert dog.night == AutoNight() and dog._operator().auto == AutoNight() and cat.night.threshold == 0.3
    assert Dog(night=True).night == NightSpec() and Dog(night=NightSpec(bloom=0.5)).night.bloom == 0.5 and Dog().night is None
    for dt in (np.float32, np.float64):
        for sp in (dog, cat):
            with pytest.raises(NotImplementedError) as e:
                sp.visualize(np.zeros((16, 16, 3), dt))
            assert "AutoNight" in str(e.value)


def test_luma_modes_refuses_what_it_does_not_take():
    from animal_vision_amd.dichromat import luma_modes

    with pytest.raises(NotImplementedError):
        luma_modes(np.zeros((4, 4, 3), np.float32))
    for shape in ((4, 4), (4, 4, 4), (0, 4, 4, 3), (2, 2, 4, 4, 3)):
        with pytest.raises(ValueError):
            luma_modes(np.zeros(shape, np.uint8))
    with pytest.raises(ValueError):
        luma_modes(np.zeros((4, 4, 3), np.uint8), threshold=1.5)


def test_video_parser_night_auto(capsys):
    from animal_vision_amd.dichromat import AutoNight, NightSpec
    from animal_vision_amd.video import make_animal, parse_args, route

    base = ["in.y4m", "out.y4m", "--species"]
    a = parse_args(base + ["Dog"])
    assert a.night_auto is False and a.night_threshold is None and a.night is False
    a = parse_args(base + ["Dog", "--night-auto"])
    assert a.night_auto is True and a.night_threshold is None and a.night is False
    dog = make_animal(a)
    assert dog.night == AutoNight(NightSpec(), 0.12) and route(dog) == "dichromat"
    a = parse_args(base + ["Cat", "--night-auto", "--night-threshold", "0.2", "--bloom", "0.12", "--batch", "4", "--depth", "2", "--split-compare"])
    assert a.night_auto and a.night_threshold == 0.2 and a.bloom == 0.12 and a.batch == 4
    assert make_animal(a).night == AutoNight(NightSpec(bloom=0.12), 0.2)
    assert parse_args(base + ["Rat", "--night-auto", "--night-threshold", "0"]).night_threshold == 0.0
    assert parse_args(base + ["Rat", "--night-auto", "--night-threshold", "1"]).night_threshold == 1.0
    assert make_animal(parse_args(base + ["Dog", "--night", "--bloom", "0.3"])).night == NightSpec(bloom=0.3)  # --night is unchanged

    def refused(argv, *words):
        with pytest.raises(SystemExit) as e:
            parse_args(argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        for w in words:
            assert w in err, (argv, err)

    refused(base + ["Dog", "--night", "--night-auto"], "--night and --night-auto exclude each other")
    refused(base + ["Dog", "--night-threshold", "0.2"], "--night-threshold needs --night-auto")
    refused(base + ["Dog", "--night", "--night-threshold", "0.2"], "--night-threshold needs --night-auto")
    refused(base + ["Dog", "--bloom", "0.12"], "--bloom needs --night: the tapetum bloom is part of the night view")
    refused(base + ["HoneyBee", "--night-auto"], "--night-auto", "HoneyBee", "not one of the 20 dichromats")
    refused(base + ["RatUV", "--night-auto", "--bloom", "0.3"], "--night-auto", "not one of the 20 dichromats")
    refused(base + ["Dog", "--night-auto", "--night-threshold", "1.5"], "--night-threshold must be at least 0 and at most 1")
    refused(base + ["Dog", "--night-auto", "--night-threshold", "-0.1"], "--night-threshold must be at least 0 and at most 1")
    refused(base + ["Dog", "--night-auto", "--night-threshold", "nan"], "--night-threshold must be at least 0 and at most 1")
    refused(base + ["Dog", "--night-auto", "--night-threshold", "dusk"], "--night-threshold takes a number")


def test_build_parser_is_what_the_golden_file_records():
    from animal_vision_amd.video import build_parser

    with open(os.path.join(GOLDEN, "video_parser.json")) as fh:
        golden = json.load(fh)
    flags = sorted(s for a in build_parser()._actions for s in a.option_strings)
    assert not [f for f in flags if f.startswith("--night") or f == "--bloom"]
    assert json.dumps(golden).count("--night") == 0  # the record knows nothing of the night options: parse_args adds them


def test_entry_points_are_declared_and_exported():
    from animal_vision_amd import _lib

    assert ctypes.sizeof(_lib.LumaModeRec) == 16 and np.dtype(_lib.LUMA_MODE_REC_DTYPE).itemsize == 16
    assert [(_lib.LumaModeRec.below.offset), _lib.LumaModeRec.max_below.offset, _lib.LumaModeRec.min_at_or_above.offset] == [0, 4, 8]
    assert [np.dtype(_lib.LUMA_MODE_REC_DTYPE).fields[n][1] for n in ("below", "max_below", "min_at_or_above")] == [0, 4, 8]
    res, args = _lib._SIGS["avx_luma_mode_u8"]
    assert res is _lib._i and len(args) == 8 and args[5] is ctypes.c_double
    res, args = _lib._SIGS["avx_dichromat_auto_u8"]
    assert res is _lib._i and len(args) == 11 and args[8] is ctypes.c_double
    assert args[6] == ctypes.POINTER(_lib.DichromatDesc) and args[7] == ctypes.POINTER(_lib.NightDesc)
    assert ctypes.sizeof(_lib.NightDesc) == 72  # NightSpec's struct is not changed
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"avx_luma_mode_u8", "avx_luma_mode_finish", "avx_dichromat_auto_u8", "avx_dichromat_night_u8", "avx_dichromat_u8"} <= syms
    assert _lib.lib.avx_abi_version() == 1
    assert _lib.lib.avx_luma_mode_u8(None, None, 1, 16, 16, 0.12, None, None) == _lib.AVX_ERR_INVALID
    assert _lib.lib.avx_dichromat_auto_u8(None, None, None, 1, 16, 16, None, None, 0.12, None, None) == _lib.AVX_ERR_INVALID
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "avx.h")).read()
    for name in ("avx_luma_mode_u8", "avx_luma_mode_finish", "avx_dichromat_auto_u8", "avx_luma_mode_rec"):
        assert name in hdr
    assert "#define AVX_ABI_VERSION 1" in hdr
