"""No GPU: the host side of the receptor distance behind the observer's acuity blur -- metrics.species_acuity against
the species' own DichromatSpec and its refusals, metrics.check_acuity at its ends, the taps against dichromat.py's, `deltae --acuity`
in the parser and in the summary line, the exported symbol with its prototype, and the yardstick of tests/_acuity_ref.py against
properties of its own definition: a 1 x 1 frame, greys, locality, the reflection against np.pad.

test_float32_figure_that_sets_the_device_bound measures what tests/test_acuity_gpu.py's tolerance rests on: the largest |float32
restatement - float64 yardstick| of the definition over that file's own frames, sizes, sigmas and observers.  On a CPU it is 2.35e-5
(Dog, the ramp at 70 x 530, sigma 1.0; four-class 1.65e-5, HoneyBee 8.1e-6); _acuity_ref.F32_FIGURE = 2.5e-5 is that figure rounded up,
and the device is held to 8 x it = 2e-4."""
import ctypes
import os

import numpy as np
import pytest

import _acuity_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSS = {"Dog": 3.5, "Squirrel": 0.7, "Elephant": 1.8, "Lion": 1.2, "Tiger": 1.2, "Bear": 1.6, "Wolf": 1.4, "Fox": 1.3, "Raccoon": 2.0, "Cat": 1.0}
DOG = ["--observer", "Dog", "--weber", "0.05,0.05"]


def _observers():
    from animal_vision_amd.metrics import Observer, observer_for

    return [observer_for("Dog", (0.05, 0.05)), observer_for("HoneyBee", (0.13, 0.06, 0.12)), Observer("four", A.FOUR, (0.08,) * 4)]


# ------------------------------------------------------------------------------------------------ the species' acuity
def test_species_acuity_is_the_specs_sigma():
    from animal_vision_amd import animals
    from animal_vision_amd.metrics import observer_names, species_acuity

    for name, sigma in GAUSS.items():
        spec = getattr(animals, name).SPEC
        assert spec.post == "gauss" and species_acuity(name) == spec.sigma == sigma, name
    assert sorted(n for n in observer_names() if n != "HoneyBee" and getattr(animals, n).SPEC.post == "gauss") == sorted(GAUSS)
    with pytest.raises(ValueError, match="Rat has no acuity blur: its rendering ends with a gain per image row"):
        species_acuity("Rat")
    for name in ("Sheep", "Pig", "Goat", "Cow", "Horse", "Rabbit", "Panda", "Deer", "Kangaroo"):
        with pytest.raises(ValueError, match=f"{name} has no single acuity: the blur of its visual streak is anisotropic and differs per image row"):
            species_acuity(name)
    with pytest.raises(ValueError, match="HoneyBee has no acuity blur"):
        species_acuity("HoneyBee")
    for bad in ("Unicorn", "dog", "RatUV", None, 3.5):
        with pytest.raises(ValueError, match="no receptor model on RGB for"):
            species_acuity(bad)


def test_check_acuity_at_its_ends():
    from animal_vision_amd.metrics import check_acuity

    assert check_acuity(0.2) == 0.2 and check_acuity(4.0) == 4.0 and check_acuity(4) == 4.0 and isinstance(check_acuity(1), float)
    assert check_acuity(np.float32(3.5)) == 3.5
    for bad in (0.19, 0.19999, 4.0000001, 4.07, 0, -1.0, float("nan"), float("inf"), True, "3.5", None):
        with pytest.raises(ValueError, match="acuity must be a finite number of pixels from 0.2 to 4"):
            check_acuity(bad)
    with pytest.raises(ValueError, match=r"got 4.07\)"):
        check_acuity(4.07)


def test_taps_are_the_species_own():
    from animal_vision_amd.dichromat import cv_auto_ksize, gaussian_taps
    from animal_vision_amd.metrics import acuity_taps

    for sigma, k in ((0.2, 3), (0.7, 7), (1.0, 9), (3.5, 29), (4.0, 33), (1.2, 11), (0.3125, 5), (0.4375, 5)):
        t = acuity_taps(sigma)
        assert t.dtype == np.float32 and len(t) == k == cv_auto_ksize(sigma) == A.ksize(sigma), sigma
        assert t.tobytes() == gaussian_taps(k, sigma).astype(np.float32).tobytes() == A.taps(sigma).astype(np.float32).tobytes(), sigma
        assert np.array_equal(A.taps(sigma), gaussian_taps(k, sigma)) and abs(A.taps(sigma).sum() - 1.0) <= 1e-15
    with pytest.raises(ValueError):
        acuity_taps(4.07)


# ------------------------------------------------------------------------------------------------ the parser and the summary
def _error(capsys, argv):
    from animal_vision_amd import deltae

    with pytest.raises(SystemExit) as e:
        deltae.parse_args(argv)
    assert e.value.code == 2, argv
    return capsys.readouterr().err


def test_acuity_in_the_parser(capsys):
    from animal_vision_amd import deltae
    from animal_vision_amd.metrics import observer_for

    ab = ["a.npy", "b.npy"]
    a = deltae.parse_args(ab + DOG + ["--acuity", "species"])  # it belongs to the statistics: valid without OUT
    assert a.acuity == 3.5 and a.observer == observer_for("Dog", (0.05, 0.05)) and a.out is None
    assert deltae.parse_args(ab + ["--observer", "Cat", "--weber", "0.1,0.1", "--acuity", "species"]).acuity == 1.0
    assert deltae.parse_args(ab + DOG + ["--acuity", "1.25"]).acuity == 1.25
    assert deltae.parse_args(ab + ["--observer", "HoneyBee", "--weber", "0.13,0.06,0.12", "--acuity", "0.2"]).acuity == 0.2
    assert deltae.parse_args(ab + ["--observer", "Sheep", "--weber", "0.1,0.1", "--acuity", "4"]).acuity == 4.0
    assert deltae.parse_args(ab + DOG).acuity is None and deltae.parse_args(ab).acuity is None
    assert "--acuity belongs to --observer" in _error(capsys, ab + ["--acuity", "1.0"])
    assert "--acuity belongs to --observer" in _error(capsys, ab + ["--acuity", "species", "--ppd", "60"])
    assert "--acuity: Rat has no acuity blur: its rendering ends with a gain per image row" in _error(capsys, ab + ["--observer", "Rat", "--weber", "0.1,0.1", "--acuity", "species"])
    assert "--acuity: Sheep has no single acuity: the blur of its visual streak is anisotropic" in _error(capsys, ab + ["--observer", "Sheep", "--weber", "0.1,0.1", "--acuity", "species"])
    assert "--acuity: HoneyBee has no acuity blur" in _error(capsys, ab + ["--observer", "HoneyBee", "--weber", "0.13,0.06,0.12", "--acuity", "species"])
    for bad in ("0.19", "4.07", "nan", "-1", "inf"):
        assert "--acuity: acuity must be a finite number of pixels from 0.2 to 4" in _error(capsys, ab + DOG + [f"--acuity={bad}"]), bad
    assert "--acuity: a number of pixels, or `species`" in _error(capsys, ab + DOG + ["--acuity", "Dog"])
    assert "--observer and --ppd do not combine" in _error(capsys, ab + DOG + ["--acuity", "species", "--ppd", "60"])
    assert "--observer needs --weber" in _error(capsys, ab + ["--observer", "Dog", "--acuity", "species"])
    help_text = deltae.build_parser().format_help()
    assert "--acuity SIGMA|species" in help_text and "Caves & Johnsen" in deltae.__doc__


def test_command_summary_and_launch_with_an_acuity(monkeypatch, capsys):
    from animal_vision_amd import deltae
    from animal_vision_amd.metrics import DeltaE, observer_for

    h = np.zeros(256, np.int64)
    h[0], h[4] = 14, 10
    monkeypatch.setattr(deltae, "stream_records", lambda args, info, fmt=None: iter([(None, DeltaE(h, 24.0, 2.25, 5, 2, 10))]))
    assert deltae.main(["a.npy", "b.npy"] + DOG + ["--acuity", "species"]) == 0
    assert "deltae: 1 frames, mean RNL dS (Dog, weber 0.05,0.05, floor 0.001, acuity 3.5 px) 1.000000, largest dS 2.250000" in capsys.readouterr().err
    assert deltae.main(["a.npy", "b.npy"] + DOG) == 0
    assert "mean RNL dS (Dog, weber 0.05,0.05, floor 0.001) 1.000000" in capsys.readouterr().err
    monkeypatch.undo()

    calls = []
    monkeypatch.setattr(deltae, "receptor_delta_launch", lambda *a, **k: calls.append(k))
    monkeypatch.setattr(deltae, "stream_map_pairs", lambda args, info, name, fmt, launch, nbytes, read: launch(None, None, None, 1, 4, 6, None, None, "s"))
    deltae.stream_records(deltae.parse_args(["a.npy", "b.npy"] + DOG + ["--acuity", "1.5", "--threshold", "2"]), {})
    deltae.stream_records(deltae.parse_args(["a.npy", "b.npy"] + DOG), {})
    dog = observer_for("Dog", (0.05, 0.05))
    assert calls[0] == dict(observer=dog, acuity=1.5, mode="heat", gain=10.0, threshold=2.0, layout="map", stream="s")
    assert calls[1] == dict(observer=dog, mode="heat", gain=10.0, threshold=1.0, layout="map", stream="s")  # without --acuity: the call it was


def test_metrics_refuse_a_bad_acuity_before_the_device(monkeypatch):
    from animal_vision_amd import metrics

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    dog = metrics.observer_for("Dog", (0.05, 0.05))
    a = np.zeros((12, 14, 3), np.uint8)
    for bad in (0.1, 4.5, float("nan"), "species"):
        for call in (lambda: metrics.receptor_delta(a, a, dog, acuity=bad), lambda: metrics.receptor_delta_map(a, a, dog, acuity=bad),
                     lambda: metrics.receptor_delta_values(a, a, dog, acuity=bad)):
            with pytest.raises(ValueError, match="acuity must be a finite number of pixels"):
                call()
    with pytest.raises(AssertionError, match="the device was asked for"):
        metrics.receptor_delta_values(a, a, dog, acuity=3.5)

    class Buf:
        ptr, nbytes = 0, 12 * 14 * 3

    class Rec:
        ptr, nbytes = 0, metrics.DELTA_E_RECORD_BYTES

    with pytest.raises(ValueError, match="acuity must be a finite number of pixels"):
        metrics.receptor_delta_launch(None, Buf(), Buf(), 1, 12, 14, None, Rec(), observer=dog, acuity=5.0)


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib

    fn = _lib.lib.avx_receptor_acuity_u8
    assert "avx_receptor_acuity_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 16
    assert fn.argtypes[6] is ctypes.POINTER(_lib.ReceptorDesc) and fn.argtypes[7] is ctypes.c_double and fn.argtypes[9] is ctypes.c_float
    assert fn(None, None, None, 1, 16, 16, None, 1.0, 0, 10.0, 1.0, 0, None, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context is refused first
    assert _lib.lib.avx_abi_version() == 1 and ctypes.sizeof(_lib.ReceptorDesc) == 144  # the observer's descriptor is not touched
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert ("int avx_receptor_acuity_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,\n"
            "                           double sigma, int mode, float gain, float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out,\n"
            "                           void* stream);") in hdr
    assert "#define AVX_ABI_VERSION 1" in hdr and "#define AVX_MAX_KSIZE 33" in hdr
    csrc = os.path.join(ROOT, "animal-vision_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "receptor_acuity.hip" in mk and "receptor_common.h" in mk
    # one copy of the value arithmetic: both kernels take it from the shared header
    for name in ("receptor.hip", "receptor_acuity.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "receptor_common.h"' in src and "Rnl<K>" in src and "logf(" not in src, name


# ------------------------------------------------------------------------------------------------ the yardstick's own properties
def test_fold_is_reflect_101():
    for n in (2, 3, 5, 17):
        x = np.arange(n) * 3 + 1
        for R in range(1, n):  # one reflection suffices: np.pad's "reflect" is BORDER_REFLECT_101
            assert np.array_equal(x[A.fold(np.arange(-R, n + R), n)], np.pad(x, R, mode="reflect")), (n, R)
    assert not A.fold(np.arange(-20, 20), 1).any()
    assert A.fold(np.arange(-7, 9), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]  # folded as often as needed
    assert A.fold(np.arange(-4, 6), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]


def test_yardstick_one_pixel_frames():
    """1 x 1: every tap folds to the one pixel, so the blurred value is (sum of taps) x lin, and dS is that of the plain distance up to
    the rounding of the taps' sum."""
    import _rnl_ref as R

    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 256, (2, 20, 1, 1, 3), dtype=np.uint8)
    for obs in _observers():
        plain = R.delta_s(a, b, obs.matrix, obs.weber, obs.floor)
        for sigma in (0.2, 1.0, 4.0):
            v = A.delta_s(a, b, obs.matrix, obs.weber, obs.floor, sigma)
            assert v.shape == (20, 1, 1) and np.abs(v - plain).max() <= 1e-9 * max(1.0, plain.max()), (obs.name, sigma)


def test_yardstick_greys_are_exactly_zero_in_float32():
    for H, W in ((5, 7), (33, 70)):
        g1, g2 = A.grey_frames(H, W)
        assert (g1 != g2).any()
        for obs in _observers():
            for sigma in (1.0, 4.0):
                assert not A.delta_s(g1, g2, obs.matrix, obs.weber, obs.floor, sigma, np.float32).any(), (obs.name, sigma)
                assert A.delta_s(g1, g2, obs.matrix, obs.weber, obs.floor, sigma).max() <= 1e-12  # float64: the three planes are equal too


def test_yardstick_locality_and_identity():
    H, W = 40, 70
    a = A.frames(33, 70)[0][0]
    a = np.concatenate([a, a[:7]])  # 40 x 70
    dog = _observers()[0]
    for sigma in (0.2, 3.5):
        R = (A.ksize(sigma) - 1) // 2
        for y, x in ((20, 35), (0, 0), (H - 1, W - 1), (3, 66)):
            b = a.copy()
            b[y, x] ^= 0x55
            for dtype in (np.float64, np.float32):
                v = A.delta_s(a, b, dog.matrix, dog.weber, dog.floor, sigma, dtype)
                near = A.near_mask(H, W, y, x, R)
                assert near[y, x] and not v[~near].any() and v[y, x] > 0, (sigma, y, x)
        assert not A.delta_s(a, a.copy(), dog.matrix, dog.weber, dog.floor, sigma, np.float32).any()
    assert A.near_mask(5, 7, 0, 0, 16).all() and A.near_mask(40, 70, 0, 0, 1).sum() == 4 and A.near_mask(40, 70, 20, 35, 14).sum() == 29 * 29


def test_blur_keeps_a_flat_frame_and_the_checkerboard_example():
    """A flat frame stays flat up to the rounding of the taps' sum; the one-pixel checkerboard blurs to its mean linear light."""
    board, flat = A.checkerboard()
    assert board.shape == flat.shape == (64, 64, 3) and len(np.unique(flat.reshape(-1, 3), axis=0)) == 1
    lin = A.blurred(flat, 3.5)
    assert np.abs(lin - lin[0, 0]).max() <= 1e-15
    dog = _observers()[0]
    import _rnl_ref as R

    plain = R.delta_s(board, flat, dog.matrix, dog.weber, dog.floor).mean()
    seen = A.delta_s(board, flat, dog.matrix, dog.weber, dog.floor, 3.5).mean()
    print(f"checkerboard, Dog (0.05, 0.05): mean dS per pixel {plain:.3f}, behind acuity 3.5 px {seen:.4f}")
    assert plain > 1 and seen < plain / 10  # on a CPU: 1.504 and 0.0430


def test_float32_figure_that_sets_the_device_bound():
    worst = {}
    for (H, W), sigmas in A.CASES.items():
        a, b = A.frames(H, W)
        for sigma in sigmas:
            for obs in _observers():
                want = A.delta_s(a, b, obs.matrix, obs.weber, obs.floor, sigma)
                got = A.delta_s(a, b, obs.matrix, obs.weber, obs.floor, sigma, np.float32)
                assert got.dtype == np.float32 and want.dtype == np.float64 and want.shape == (len(A.KINDS), H, W)
                d = float(np.abs(got.astype(np.float64) - want).max())
                worst[obs.name] = max(worst.get(obs.name, 0.0), d)
                print(f"acuity float32 restatement {H}x{W} sigma {sigma} {obs.name}: largest |float32 - float64| {d:.3e}, largest dS {want.max():.3f}")
    figure = max(worst.values())
    print(f"the float32 figure: {figure:.3e} ({', '.join(f'{k} {v:.2e}' for k, v in worst.items())}); F32_FIGURE {A.F32_FIGURE:g}, the device's bound {A.BOUND:g}")
    assert figure <= A.F32_FIGURE < 1.25e-4 and A.BOUND == 8 * A.F32_FIGURE <= 1e-3
