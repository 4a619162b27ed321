"""No GPU: the host side of the receptor-noise-limited colour distance -- the yardstick of tests/_rnl_ref.py against hand
values of its own definition, the observers of metrics.observer_for against dichromat.py's matrix and HoneybeeOp.rgb_matrix, the
refusals of metrics.Observer, `deltae --observer` in the parser, the argument checks that need no device, the exported symbol with its
prototype and descriptor, and the command's summary line with the device loop stubbed."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest

import _rnl_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICHROMATS = ["Cat", "Dog", "Sheep", "Pig", "Goat", "Cow", "Horse", "Rabbit", "Panda", "Squirrel", "Elephant", "Lion", "Wolf", "Fox", "Bear", "Raccoon",
              "Deer", "Kangaroo", "Tiger", "Rat"]
BEE_WEBER = (0.13, 0.06, 0.12)


# ------------------------------------------------------------------------------------------------ the yardstick
def _catches_for(df, floor):
    """Catches (qa, qb) whose contrasts are df: qb = 0.5 in every class, qa + floor = (qb + floor) exp(df)."""
    df = np.asarray(df, np.float64)
    qb = np.full(df.shape, 0.5)
    return (qb + floor) * np.exp(df) - floor, qb


def _pairwise(df, e):
    """The equal-noise form: sqrt(sum_{i<j} (df_i - df_j)^2 / (K e^2)) -- for K = 2 this is |df_1 - df_2| / sqrt(2 e^2)."""
    K = len(df)
    return math.sqrt(sum((df[i] - df[j]) ** 2 for i, j in itertools.combinations(range(K), 2)) / (K * e * e))


def test_hand_values_of_delta_s_from_catches():
    qa, qb = _catches_for([0.1, 0.0], 1e-3)
    assert abs(R.delta_s_from_catches(qa, qb, (0.05, 0.05), 1e-3) - 0.1 / math.sqrt(0.005)) <= 1e-12
    for df, e in (([0.3, -0.2, 0.05], 0.08), ([0.0, 0.4, 0.4], 0.2), ([0.3, -0.2, 0.05, 0.11], 0.08), ([1.0, 0.0, 0.0, -1.0], 0.5)):
        qa, qb = _catches_for(df, 1e-3)
        got = float(R.delta_s_from_catches(qa, qb, (e,) * len(df), 1e-3))
        assert abs(got - _pairwise(df, e)) <= 1e-12 * max(1.0, got), (df, e, got)
    # unequal noise, K = 3, written out from the definition
    df, e = [0.2, -0.1, 0.4], (0.13, 0.06, 0.12)
    qa, qb = _catches_for(df, 1e-3)
    num = e[0] ** 2 * (df[2] - df[1]) ** 2 + e[1] ** 2 * (df[2] - df[0]) ** 2 + e[2] ** 2 * (df[1] - df[0]) ** 2
    den = (e[0] * e[1]) ** 2 + (e[0] * e[2]) ** 2 + (e[1] * e[2]) ** 2
    assert abs(float(R.delta_s_from_catches(qa, qb, e, 1e-3)) - math.sqrt(num / den)) <= 1e-12
    # and K = 4
    df, e = [0.2, -0.1, 0.4, 0.05], (0.1, 0.07, 0.05, 0.2)
    qa, qb = _catches_for(df, 1e-3)
    num = sum((e[k] * e[l]) ** 2 * (df[i] - df[j]) ** 2 for (i, j), (k, l) in (((3, 2), (0, 1)), ((3, 1), (0, 2)), ((2, 1), (0, 3)), ((3, 0), (1, 2)),
                                                                                 ((2, 0), (1, 3)), ((1, 0), (2, 3))))
    den = sum(np.prod([e[k] ** 2 for k in range(4) if k != out]) for out in range(4))
    assert abs(float(R.delta_s_from_catches(qa, qb, e, 1e-3)) - math.sqrt(num / den)) <= 1e-12


def test_a_constant_added_to_every_contrast_changes_nothing():
    """Brightness: scaling every (catch + floor) of one side by one factor adds one constant to every df_i."""
    rng = np.random.default_rng(3)
    for K, e in ((2, (0.05, 0.2)), (3, BEE_WEBER), (4, (0.08,) * 4)):
        df = rng.uniform(-1, 1, (50, K))
        qa, qb = _catches_for(df, 1e-3)
        qa2, _ = _catches_for(df + 0.7, 1e-3)
        want = R.delta_s_from_catches(qa, qb, e, 1e-3)
        assert np.abs(R.delta_s_from_catches(qa2, qb, e, 1e-3) - want).max() <= 1e-11 and want.min() > 0
    assert float(R.delta_s_from_catches([0.3, 0.3, 0.3], [0.9, 0.9, 0.9], BEE_WEBER, 1e-3)) == 0.0


def test_delta_s_of_pixels_greys_equal_codes_and_float32():
    rng = np.random.default_rng(4)
    from animal_vision_amd.metrics import observer_for

    for obs in (observer_for("Dog", (0.05, 0.05)), observer_for("HoneyBee", BEE_WEBER)):
        a = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
        b = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
        b[:5] = a[:5]
        v = R.delta_s(a, b, obs.matrix, obs.weber, obs.floor)
        assert v.dtype == np.float64 and v.shape == (40, 50) and not v[:5].any() and v[5:].min() > 0
        g1, g2 = np.repeat(rng.integers(0, 256, (40, 50, 1), dtype=np.uint8), 3, axis=2), np.repeat(rng.integers(0, 256, (40, 50, 1), dtype=np.uint8), 3, axis=2)
        assert not R.delta_s(g1, g2, obs.matrix, obs.weber, obs.floor).any()  # the measure is chromatic
        assert not R.delta_s(g1, g2, obs.matrix, obs.weber, obs.floor, dtype=np.float32).any()
        v32 = R.delta_s(a, b, obs.matrix, obs.weber, obs.floor, dtype=np.float32)
        assert v32.dtype == np.float32 and np.abs(v32 - v).max() <= 2e-4
        q = R.catches(np.array([[255, 255, 255]], np.uint8), obs.matrix)
        assert np.abs(q - 1.0).max() <= 1e-15  # white has catch 1 in every class


# ------------------------------------------------------------------------------------------------ observers
def test_observers_of_the_species():
    from animal_vision_amd import animals
    from animal_vision_amd.dichromat import M_RGB_TO_LMS
    from animal_vision_amd.metrics import Observer, observer_for, observer_names

    lms = M_RGB_TO_LMS.astype(np.float64)
    dog = observer_for("Dog", (0.05, 0.05))
    alpha = animals.Dog.SPEC.alpha
    assert isinstance(dog, Observer) and dog.name == "Dog" and dog.n_receptors == 2 and dog.weber == (0.05, 0.05) and dog.floor == 1e-3
    assert np.array_equal(np.array(dog.matrix), np.stack([alpha * lms[0] + (1 - alpha) * lms[1], lms[2]])) and alpha == 0.58
    assert observer_for(animals.Dog, (0.05, 0.05)) == dog and observer_for(animals.Dog(), [0.05, 0.05]) == dog
    assert observer_for("Dog", (0.05, 0.05), 0.01).floor == 0.01
    bee = observer_for("HoneyBee", BEE_WEBER)
    assert bee.n_receptors == 3 and np.array_equal(np.array(bee.matrix), animals.HoneyBee()._operator().rgb_matrix.astype(np.float64))
    assert observer_for(animals.HoneyBee, BEE_WEBER) == bee and observer_for(animals.HoneyBee(), BEE_WEBER) == bee
    assert observer_names() == DICHROMATS + ["HoneyBee"] and len(observer_names()) == 21
    for name in DICHROMATS:
        o = observer_for(name, (0.1, 0.2))
        a = getattr(animals, name).SPEC.alpha
        assert o.name == name and np.array_equal(np.array(o.matrix), np.stack([a * lms[0] + (1 - a) * lms[1], lms[2]])), name
    for bad in ("Mantis Shrimp", "RatUV", "ReinDeer", "Unicorn", animals.MantisShrimp, animals.RatUV(), 7):
        with pytest.raises(ValueError, match="no receptor model on RGB for '?(Mantis Shrimp|MantisShrimp|RatUV|ReinDeer|Unicorn|int)"):
            observer_for(bad, (0.1, 0.1))
    with pytest.raises(AttributeError):  # dataclasses.FrozenInstanceError
        dog.floor = 0.5
    d = dog.desc()
    assert (d.struct_size, d.n_receptors, d.floor) == (144, 2, 1e-3) and list(d.matrix)[:6] == [v for row in dog.matrix for v in row]
    assert list(d.weber) == [0.05, 0.05, 0.0, 0.0] and dog.describe() == "Dog, weber 0.05,0.05, floor 0.001"


def test_observer_refusals():
    from animal_vision_amd.metrics import Observer

    m2, m3 = [[0.2, 0.7, 0.1], [0.0, 0.1, 0.9]], [[0.2, 0.7, 0.1], [0.0, 0.1, 0.9], [0.5, 0.5, 0.0]]
    assert Observer("x", m2, (0.01, 1.0), 1e-6).n_receptors == 2 and Observer("x", m3 + [[1, 0, 0]], (0.1,) * 4, 0.1).n_receptors == 4
    for e in (0.009, 1.01, float("nan"), -0.1, "0.1", True):
        with pytest.raises(ValueError, match=r"weber\[1\] must be a number from 0.01 to 1"):
            Observer("x", m2, (0.05, e))
    for fl in (0, 0.2, float("nan"), -1e-3, "1e-3"):
        with pytest.raises(ValueError, match="floor must be a number from 1e-06 to 0.1"):
            Observer("x", m2, (0.05, 0.05), fl)
    with pytest.raises(ValueError, match="matrix entries must be finite and not negative"):
        Observer("x", [[0.2, -0.1, 0.9], [0, 0, 1]], (0.05, 0.05))
    with pytest.raises(ValueError, match="matrix entries must be finite"):
        Observer("x", [[0.2, float("inf"), 0.9], [0, 0, 1]], (0.05, 0.05))
    with pytest.raises(ValueError, match="matrix row 1 sums to 0"):
        Observer("x", [[0.2, 0.1, 0.9], [0, 0, 0]], (0.05, 0.05))
    for m, e in (([[1, 1, 1]], (0.05,)), (m3 + m2, (0.05,) * 5)):  # K = 1 and K = 5
        with pytest.raises(ValueError, match="K = 2, 3 or 4 receptor classes"):
            Observer("x", m, e)
    with pytest.raises(ValueError, match="matrix must be K x 3"):
        Observer("x", [[1, 1], [1, 1]], (0.05, 0.05))
    for e in ((0.05,), (0.05,) * 3, 0.05, "0.05,0.05"):
        with pytest.raises(ValueError, match="weber must hold one Weber fraction per receptor class, 2"):
            Observer("x", m2, e)


# ------------------------------------------------------------------------------------------------ the parser
def _error(capsys, argv):
    from animal_vision_amd import deltae

    with pytest.raises(SystemExit) as e:
        deltae.parse_args(argv)
    assert e.value.code == 2, argv
    return capsys.readouterr().err


def test_observer_in_the_parser(capsys):
    from animal_vision_amd import deltae
    from animal_vision_amd.metrics import observer_for

    a = deltae.parse_args(["a.npy", "b.npy", "--observer", "Dog", "--weber", "0.05,0.05"])  # it belongs to the statistics: valid without OUT
    assert a.observer == observer_for("Dog", (0.05, 0.05)) and a.out is None and a.ppd is None
    assert (a.mode, a.gain, a.threshold, a.layout) == ("heat", 10.0, 1.0, "map")
    a = deltae.parse_args(["a.npy", "b.npy", "o.npy", "--observer", "HoneyBee", "--weber", "0.13,0.06,0.12", "--floor", "0.01", "--layout", "side", "--threshold", "3"])
    assert a.observer == observer_for("HoneyBee", BEE_WEBER, 0.01) and (a.out, a.layout, a.threshold) == ("o.npy", "side", 3.0)
    assert deltae.parse_args(["a.npy", "b.npy"]).observer is None and deltae.parse_args(["a.npy", "b.npy", "--ppd", "60"]).observer is None
    ab = ["a.npy", "b.npy"]
    assert "--observer needs --weber" in _error(capsys, ab + ["--observer", "Dog"])
    assert "--weber belongs to --observer" in _error(capsys, ab + ["--weber", "0.05,0.05"])
    assert "--floor belongs to --observer" in _error(capsys, ab + ["--floor", "0.01"])
    assert "weber must hold one Weber fraction per receptor class, 2" in _error(capsys, ab + ["--observer", "Dog", "--weber", "0.05"])
    assert "weber must hold one Weber fraction per receptor class, 2" in _error(capsys, ab + ["--observer", "Cat", "--weber", "0.05,0.05,0.05"])
    assert "weber must hold one Weber fraction per receptor class, 3" in _error(capsys, ab + ["--observer", "HoneyBee", "--weber", "0.05,0.05"])
    assert "--observer and --ppd do not combine" in _error(capsys, ab + ["--observer", "Dog", "--weber", "0.05,0.05", "--ppd", "60"])
    for name in ("Mantis Shrimp", "RatUV", "ReinDeer", "dog", "Unicorn"):
        err = _error(capsys, ab + ["--observer", name, "--weber", "0.05,0.05"])
        assert f"--observer: no receptor model on RGB for {name!r}" in err and "HoneyBee" in err, name
    assert "--weber: comma-separated numbers" in _error(capsys, ab + ["--observer", "Dog", "--weber", "0.05,x"])
    assert "weber[1] must be a number from 0.01 to 1" in _error(capsys, ab + ["--observer", "Dog", "--weber", "0.05,0.009"])
    assert "weber[0] must be a number from 0.01 to 1" in _error(capsys, ab + ["--observer", "Dog", "--weber", "1.01,0.05"])
    for fl in ("0", "0.2", "nan"):
        assert "floor must be a number from 1e-06 to 0.1" in _error(capsys, ab + ["--observer", "Dog", "--weber", "0.05,0.05", f"--floor={fl}"])
    assert "--mode shapes the video that OUT names" in _error(capsys, ab + ["--observer", "Dog", "--weber", "0.05,0.05", "--mode", "plain"])
    help_text = deltae.build_parser().format_help()
    assert "--observer" in help_text and "--weber" in help_text and "--floor" in help_text and "0.13,0.06,0.12" in help_text
    assert "Vorobyev & Osorio" in deltae.__doc__ and deltae.CSV_HEADER == "frame,de_mean,de_p50,de_p95,de_max,x,y,beyond"


# ------------------------------------------------------------------------------------------------ metrics.receptor_delta* without a device
def test_receptor_delta_refuses_bad_arguments_before_the_device(monkeypatch):
    from animal_vision_amd import metrics

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    dog = metrics.observer_for("Dog", (0.05, 0.05))
    a = np.zeros((12, 14, 3), np.uint8)
    with pytest.raises(ValueError, match=r"\(12, 14, 3\).*\(12, 15, 3\)"):
        metrics.receptor_delta_map(a, np.zeros((12, 15, 3), np.uint8), dog)
    with pytest.raises(ValueError, match="uint8"):
        metrics.receptor_delta_values(a.astype(np.uint16), a, dog)
    for obs in ("Dog", None, (0.05, 0.05)):
        for call in (lambda: metrics.receptor_delta(a, a, obs), lambda: metrics.receptor_delta_map(a, a, obs), lambda: metrics.receptor_delta_values(a, a, obs)):
            with pytest.raises(ValueError, match="observer must be an Observer"):
                call()
    for kw, msg in ((dict(mode="abs"), "mode must be one of heat, plain"), (dict(layout="top"), "layout must be one of map, side"),
                    (dict(threshold=-1.0), "threshold must be finite and at least 0"), (dict(gain=0), "gain must be above 0 and at most 255")):
        with pytest.raises(ValueError, match=msg):
            metrics.receptor_delta_map(a, a, dog, **kw)
    with pytest.raises(ValueError, match="threshold must be finite and at least 0"):
        metrics.receptor_delta(a, a, dog, -1)
    for call in (lambda: metrics.receptor_delta(a, a, dog), lambda: metrics.receptor_delta(a, a, dog, 2.5), lambda: metrics.receptor_delta_values(a, a, dog),
                 lambda: metrics.receptor_delta_map(a, a, dog, mode="plain", gain=255, threshold=0, layout="side")):
        with pytest.raises(AssertionError, match="the device was asked for"):
            call()

    class Buf:
        ptr, nbytes = 0, 12 * 14 * 3

    class Rec:
        ptr, nbytes = 0, metrics.DELTA_E_RECORD_BYTES

    with pytest.raises(ValueError, match="side frames need"):
        metrics.receptor_delta_launch(None, Buf(), Buf(), 1, 12, 14, Buf(), Rec(), observer=dog, layout="side")
    with pytest.raises(ValueError, match="records need"):
        metrics.receptor_delta_launch(None, Buf(), Buf(), 1, 12, 14, None, Buf(), observer=dog)
    with pytest.raises(ValueError, match="the values of 1 frames need"):
        metrics.receptor_delta_launch(None, Buf(), Buf(), 1, 12, 14, None, Rec(), observer=dog, d_float=Buf())
    with pytest.raises(ValueError, match="observer must be an Observer"):
        metrics.receptor_delta_launch(None, Buf(), Buf(), 1, 12, 14, None, Rec(), observer="Dog")
    with pytest.raises(ValueError):
        metrics.receptor_delta_launch(None, Buf(), Buf(), 17, 12, 14, None, Rec(), observer=dog)


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib

    fn = _lib.lib.avx_receptor_delta_u8
    assert "avx_receptor_delta_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    assert fn.argtypes[6] is ctypes.POINTER(_lib.ReceptorDesc) and fn.argtypes[8] is ctypes.c_float and fn.argtypes[9] is ctypes.c_float
    D = _lib.ReceptorDesc
    assert ctypes.sizeof(D) == 144 and [(n, getattr(D, n).offset) for n, _ in D._fields_] == [("struct_size", 0), ("n_receptors", 4), ("matrix", 8),
                                                                                             ("weber", 104), ("floor", 136)]
    assert fn(None, None, None, 1, 16, 16, None, 0, 10.0, 1.0, 0, None, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context is refused first
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert ("int avx_receptor_delta_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, const avx_receptor_desc* obs, int mode,\n"
            "                          float gain, float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out, void* stream);") in hdr
    for field in ("uint32_t struct_size;", "int32_t n_receptors;", "double matrix[12];", "double weber[4];", "double floor;"):
        assert field in hdr, field
    assert "#define AVX_ABI_VERSION 1" in hdr
    csrc = os.path.join(ROOT, "animal-vision_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "receptor.hip" in mk and "delta_e_walk.h" in mk
    # one chunk walk for both kernels: neither file carries its own copy
    for name in ("delta_e.hip", "receptor.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "delta_e_walk.h"' in src and "de_chunk_walk<VEC>" in src and "__shared__" not in src and "de_record_share(" not in src, name


# ------------------------------------------------------------------------------------------------ the command, the device loop stubbed
def test_command_summary_and_launch_with_an_observer(monkeypatch, capsys):
    from animal_vision_amd import deltae
    from animal_vision_amd.metrics import DeltaE, observer_for

    h = np.zeros(256, np.int64)
    h[0], h[4], h[20] = 12, 10, 2
    items = [(None, DeltaE(h, 48.0, 10.25, 5, 2, 12)), (None, DeltaE(h, 36.0, 10.25, 1, 1, 12))]
    seen = {}

    def stub(args, info, fmt=None):
        seen["observer"] = args.observer
        info["hw"] = (4, 6)
        yield from items

    monkeypatch.setattr(deltae, "stream_records", stub)
    status = deltae.main(["a.npy", "b.npy", "--observer", "Dog", "--weber", "0.05,0.05"])
    cap = capsys.readouterr()
    assert status == 0 and seen["observer"] == observer_for("Dog", (0.05, 0.05))
    assert cap.out.splitlines() == ["frame,de_mean,de_p50,de_p95,de_max,x,y,beyond", "0,2.000000,0.500000,10.500000,10.250000,5,2,12",
                                    "1,1.500000,0.500000,10.500000,10.250000,1,1,12"]
    assert "deltae: 2 frames, mean RNL dS (Dog, weber 0.05,0.05, floor 0.001) 1.750000, largest dS 10.250000 (frame 0, pixel x 5 y 2), 24 pixels beyond 1," in cap.err
    status = deltae.main(["a.npy", "b.npy", "--observer", "HoneyBee", "--weber", "0.13,0.06,0.12", "--floor", "0.01", "--max-mean", "1.75"])
    cap = capsys.readouterr()
    assert status == 1 and "mean RNL dS (HoneyBee, weber 0.13,0.06,0.12, floor 0.01) 1.750000" in cap.err and "deltae: frame 0: mean dE 2.000000 is above --max-mean 1.75" in cap.err
    monkeypatch.undo()

    calls = []
    monkeypatch.setattr(deltae, "delta_e_launch", lambda *a, **k: calls.append(("plain", k)))
    monkeypatch.setattr(deltae, "scielab_launch", lambda *a, **k: calls.append(("scielab", k)))
    monkeypatch.setattr(deltae, "receptor_delta_launch", lambda *a, **k: calls.append(("receptor", k)))
    monkeypatch.setattr(deltae, "stream_map_pairs", lambda args, info, name, fmt, launch, nbytes, read: launch(None, None, None, 1, 4, 6, None, None, "s"))
    deltae.stream_records(deltae.parse_args(["a.npy", "b.npy"]), {})
    deltae.stream_records(deltae.parse_args(["a.npy", "b.npy", "--observer", "Dog", "--weber", "0.05,0.05", "--threshold", "2"]), {})
    assert [c[0] for c in calls] == ["plain", "receptor"]
    assert calls[1][1] == dict(observer=observer_for("Dog", (0.05, 0.05)), mode="heat", gain=10.0, threshold=2.0, layout="map", stream="s")
