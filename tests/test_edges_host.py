"""No GPU: the host side of receptor contrast within a frame -- closed forms of the yardstick of tests/_edges_ref.py (a
two-colour frame, two greys, 1 x 1, the skipped neighbours, symmetry, transposes), the `edges` parser with every option and refusal,
the Python entries' refusals before any device work, and the exported symbol with its prototype.

test_float32_figure_that_sets_the_device_bound measures what tests/test_edges_gpu.py's tolerance rests on: the largest |float32
restatement - float64 yardstick| of the definition over that file's own frames, sizes, sigmas, steps, observers and channels.  On a CPU
it is 2.30e-5 (Dog, chromatic, the ramp at 70 x 530 without blur, step 1; the four-class observer's largest is 1.43e-5, HoneyBee's
8.9e-6; the values reach 86.4); _edges_ref.F32_FIGURE = 2.5e-5 is that figure rounded up, and the device is held to 8 x it = 2e-4."""
import ctypes
import math
import os

import numpy as np
import pytest

import _acuity_ref as A
import _edges_ref as E
from _deltae_ref import decode_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOG = ["--observer", "Dog", "--weber", "0.05,0.05"]
BEE = ["--observer", "HoneyBee", "--weber", "0.13,0.06,0.12"]
IN = "synthetic:64x48:3"


def _observers():
    from animal_vision_amd.metrics import Observer, observer_for

    return [observer_for("Dog", (0.05, 0.05)), observer_for("HoneyBee", (0.13, 0.06, 0.12)), Observer("four", A.FOUR, (0.08,) * 4)]


def _values(frame, obs, channel="chromatic", sigma=0.0, step=1, dtype=np.float64):
    return E.values(frame, obs.matrix, obs.weber, obs.floor, E.ACHROMATIC[obs.name], channel, sigma, step, dtype)


def split_frame(H, W, c, left, right):
    f = np.empty((H, W, 3), np.uint8)
    f[:, :c], f[:, c:] = left, right
    return f


# ------------------------------------------------------------------------------------------------ closed forms of the yardstick
@pytest.mark.parametrize("D", [1, 2, 8])
def test_two_colours_split_at_a_column(D):
    """Without blur dS(colour 1, colour 2) stands in the columns c - D .. c + D - 1 and 0 elsewhere."""
    from _rnl_ref import delta_s

    H, W, c = 11, 40, 17
    c1, c2 = (200, 60, 60), (60, 200, 60)
    for obs in _observers():
        for dtype in (np.float64, np.float32):
            v = _values(split_frame(H, W, c, c1, c2), obs, "chromatic", 0.0, D, dtype)
            band = np.zeros((H, W), bool)
            band[:, c - D : c + D] = True
            assert not v[~band].any() and (v[band] == v[0, c]).all() and v[0, c] > 1, (obs.name, D)
        want = float(delta_s(np.array(c1, np.uint8), np.array(c2, np.uint8), obs.matrix, obs.weber, obs.floor))
        assert abs(float(_values(split_frame(H, W, c, c1, c2), obs, "chromatic", 0.0, D)[0, c]) - want) <= 1e-12 * want, (obs.name, D)


@pytest.mark.parametrize("D", [1, 2, 8])
def test_two_greys_split_at_a_column(D):
    """g1 | g2: the achromatic value is |ln((g1 + eps) / (g2 + eps))| / e_L on the same columns, the chromatic value exactly 0."""
    H, W, c = 9, 40, 23
    lut = decode_table()
    for g1, g2 in ((40, 200), (0, 255), (128, 129)):
        f = split_frame(H, W, c, (g1,) * 3, (g2,) * 3)
        for obs in _observers():
            e_l = E.ACHROMATIC[obs.name][1]
            want = abs(math.log((lut[g1] + obs.floor) / (lut[g2] + obs.floor))) / e_l
            band = np.zeros((H, W), bool)
            band[:, c - D : c + D] = True
            for dtype in (np.float64, np.float32):
                assert not _values(f, obs, "chromatic", 0.0, D, dtype).any(), (obs.name, g1, g2)
                v = _values(f, obs, "achromatic", 0.0, D, dtype)
                assert not v[~band].any() and (v[band] == v[0, c]).all(), (obs.name, g1, g2)
                assert np.array_equal(_values(f, obs, "either", 0.0, D, dtype), v)
            assert abs(float(_values(f, obs, "achromatic", 0.0, D)[0, c]) - want) <= 1e-9 * want, (obs.name, g1, g2, D)


def test_one_pixel_frames_and_skipped_neighbours():
    for obs in _observers():
        for sigma, D in E.CASES[(1, 1)]:
            for ch in E.CHANNELS:
                assert not _values(E.frames(1, 1), obs, ch, sigma, D).any()
        # H <= D and W <= D: no neighbour inside the frame
        assert not _values(E.frames(5, 7), obs, "either", 0.0, 8).any()
        # a neighbour outside the frame is skipped, not reflected: in a 1 x 9 row at step 8 only the two ends see each other
        row = E.frames(1, 9)[0]
        v = _values(row, obs, "either", 0.0, 8)
        assert v[0, 0] == v[0, 8] > 0 and not v[0, 1:8].any()
        # and a pixel whose only differing neighbour would be its own reflection is 0
        f = np.zeros((1, 3, 3), np.uint8)
        f[0, 1] = (255, 0, 0)
        assert not _values(f, obs, "either", 0.0, 2).any() and _values(f, obs, "either", 0.0, 1).all()


def test_symmetry_transpose_and_mirror():
    f = E.frames(16, 16)[0]
    for obs in _observers():
        for ch in E.CHANNELS:
            v = _values(f, obs, ch, 0.0, 2, np.float32)
            assert np.array_equal(_values(f.transpose(1, 0, 2), obs, ch, 0.0, 2, np.float32), v.T)
            assert np.array_equal(_values(f[:, ::-1], obs, ch, 0.0, 2, np.float32), v[:, ::-1])
            assert np.array_equal(_values(f[::-1], obs, ch, 0.0, 2, np.float32), v[::-1])
        # v(p, n) = v(n, p) bit for bit, in float32 too
        fl = E.log_catches(E.linear(f, 1.0, np.float32), [list(r) for r in obs.matrix] + [list(E.luminance_row(obs.matrix, E.ACHROMATIC[obs.name][0]))],
                           obs.floor, np.float32)
        p, n = fl[:, :-3], fl[:, 3:]
        for ch in E.CHANNELS:
            e_l = E.ACHROMATIC[obs.name][1]
            assert np.array_equal(E.pair_value(p, n, obs.weber, e_l, ch, np.float32), E.pair_value(n, p, obs.weber, e_l, ch, np.float32))
        # either is the element-wise larger of the two
        both = [_values(f, obs, ch, 1.0, 1, np.float32) for ch in E.CHANNELS]
        assert np.array_equal(both[2], np.maximum(both[0], both[1]))


def test_flat_frames_and_greys():
    flat = np.broadcast_to(np.array((200, 60, 60), np.uint8), (12, 20, 3))
    g = A.grey_frames(12, 20)[0]
    for obs in _observers():
        for sigma in (0.0, 1.0, 4.0):
            for dtype in (np.float64, np.float32):
                assert not _values(g, obs, "chromatic", sigma, 1, dtype).any(), (obs.name, sigma)
            assert _values(g, obs, "achromatic", sigma, 1).any()
        for ch in E.CHANNELS:
            assert not _values(flat, obs, ch, 0.0, 1, np.float32).any()


def test_luminance_row_is_the_mean_of_the_normalised_rows():
    from animal_vision_amd.metrics import check_achromatic

    for obs in _observers():
        classes, e_l = E.ACHROMATIC[obs.name]
        d = check_achromatic(obs, (classes, e_l))
        assert d.struct_size == ctypes.sizeof(type(d)) == 40 and d.weber == e_l
        assert np.array_equal(np.array(d.row[:]), E.luminance_row(obs.matrix, classes)) and abs(sum(d.row[:]) - 1) < 1e-15
    assert check_achromatic(_observers()[0], None) is None


# ------------------------------------------------------------------------------------------------ the float32 figure
def test_float32_figure_that_sets_the_device_bound():
    worst = {}
    largest = 0.0
    for (H, W), cases in E.CASES.items():
        f = E.frames(H, W)
        for sigma, D in cases:
            for obs in _observers():
                for ch in E.CHANNELS:
                    want = E.values(f, obs.matrix, obs.weber, obs.floor, E.ACHROMATIC[obs.name], ch, sigma, D, key=(H, W))
                    got = E.values(f, obs.matrix, obs.weber, obs.floor, E.ACHROMATIC[obs.name], ch, sigma, D, np.float32, key=(H, W))
                    assert got.dtype == np.float32 and want.dtype == np.float64 and want.shape == (len(E.KINDS), H, W)
                    d = float(np.abs(got.astype(np.float64) - want).max())
                    worst[obs.name] = max(worst.get(obs.name, 0.0), d)
                    largest = max(largest, float(want.max()))
                    print(f"edges float32 restatement {H}x{W} sigma {sigma} step {D} {obs.name} {ch}: largest |float32 - float64| {d:.3e}, "
                          f"largest value {want.max():.3f}")
    figure = max(worst.values())
    print(f"the float32 figure: {figure:.3e} ({', '.join(f'{k} {v:.2e}' for k, v in worst.items())}); largest value {largest:.1f}; "
          f"F32_FIGURE {E.F32_FIGURE:g}, the device's bound {E.BOUND:g}")
    assert figure <= E.F32_FIGURE < 1.25e-4 and E.BOUND == 8 * E.F32_FIGURE <= 1e-3


def test_cases_cover_what_the_kernel_can_get_wrong():
    assert list(E.CASES) == [(1, 1), (1, 9), (2, 3), (5, 7), (16, 16), (33, 70), (70, 530), (96, 160)]
    pairs = {c for cases in E.CASES.values() for c in cases}
    assert {s for s, _ in pairs} == {0.0, 0.2, 1.0, 3.5, 4.0} and {d for _, d in pairs} == {1, 2, 8}
    assert (3.5, 8) in E.CASES[(33, 70)] and sorted(E.ACHROMATIC) == ["Dog", "HoneyBee", "four"]


# ------------------------------------------------------------------------------------------------ the parser and the summary
def _error(capsys, argv):
    from animal_vision_amd import edges

    with pytest.raises(SystemExit) as e:
        edges.parse_args(argv)
    assert e.value.code == 2, argv
    return capsys.readouterr().err


def test_every_option_in_the_parser():
    from animal_vision_amd import edges
    from animal_vision_amd.metrics import observer_for

    a = edges.parse_args([IN] + DOG)
    assert a.observer == observer_for("Dog", (0.05, 0.05)) and a.out is None and a.achromatic is None and a.channel == "chromatic"
    assert (a.acuity, a.step, a.mode, a.gain, a.threshold, a.batch, a.depth, a.csv) == (None, 1, "heat", 10.0, 1.0, 8, 2, None)
    assert edges.describe(a) == "Dog, weber 0.05,0.05, floor 0.001, step 1"
    a = edges.parse_args([IN, "o.y4m"] + DOG + ["--achromatic", "1:0.1", "--channel", "either", "--acuity", "species", "--floor", "0.01", "--step", "8",
                                               "--mode", "plain", "--gain", "4", "--threshold", "0.5", "--csv", "f.csv", "--batch", "16", "--depth", "8"])
    assert a.achromatic == ((1,), 0.1) and a.channel == "either" and a.acuity == 3.5 and a.observer.floor == 0.01 and a.out == "o.y4m"
    assert (a.step, a.mode, a.gain, a.threshold, a.csv, a.batch, a.depth) == (8, "plain", 4.0, 0.5, "f.csv", 16, 8)
    assert edges.describe(a) == "Dog, weber 0.05,0.05, floor 0.01, achromatic 1:0.1, channel either, acuity 3.5 px, step 8"
    a = edges.parse_args([IN] + DOG + ["--achromatic", "1:0.1", "--acuity", "species"])
    assert a.channel == "either"  # the default with a luminance channel
    assert edges.describe(a) == "Dog, weber 0.05,0.05, floor 0.001, achromatic 1:0.1, acuity 3.5 px, step 1"
    a = edges.parse_args([IN] + BEE + ["--achromatic", "3:0.12", "--channel", "chromatic", "--acuity", "1.25"])
    assert a.achromatic == ((3,), 0.12) and a.channel == "chromatic" and a.acuity == 1.25 and a.observer.n_receptors == 3
    assert edges.parse_args([IN] + BEE + ["--achromatic", "2+3:0.12", "--channel", "achromatic"]).achromatic == ((2, 3), 0.12)
    a = edges.parse_args(["clip.yuv", "maps/", "--pix-fmt", "nv12", "--size", "64x48", "--scale", "32x24", "--range", "full", "--matrix", "bt709",
                          "--out-pix-fmt", "yuv420p"] + DOG)
    assert (a.pix_fmt, a.size, a.scale, a.range, a.matrix, a.out_pix_fmt) == ("nv12", (64, 48), (32, 24), "full", "bt709", "yuv420p")
    help_text = edges.build_parser().format_help()
    for flag in ("--observer NAME", "--weber E1,E2[,E3]", "--floor EPS", "--achromatic CLASSES:E", "--channel {chromatic,achromatic,either}",
                 "--acuity SIGMA|species", "--step D", "--mode {heat,plain}", "--gain G", "--threshold T", "--csv FILE", "--batch N", "--depth"):
        assert flag in help_text, flag
    assert "van den Berg" in edges.__doc__


def test_every_refusal_in_the_parser(capsys):
    assert "--observer NAME is required" in _error(capsys, [IN])
    assert "--observer needs --weber" in _error(capsys, [IN, "--observer", "Dog"])
    assert "weber must hold one Weber fraction per receptor class, 2" in _error(capsys, [IN, "--observer", "Dog", "--weber", "0.05"])
    assert "weber must hold one Weber fraction per receptor class, 3" in _error(capsys, [IN, "--observer", "HoneyBee", "--weber", "0.1,0.1"])
    assert "--weber: comma-separated numbers" in _error(capsys, [IN, "--observer", "Dog", "--weber", "a,b"])
    assert "--observer: no receptor model on RGB for 'MantisShrimp'" in _error(capsys, [IN, "--observer", "MantisShrimp", "--weber", "0.1,0.1"])
    for ch in ("achromatic", "either"):
        assert f"--channel {ch} needs --achromatic" in _error(capsys, [IN] + DOG + ["--channel", ch])
    assert "--achromatic: class 3 is not one of Dog's receptor classes 1..2" in _error(capsys, [IN] + DOG + ["--achromatic", "3:0.1"])
    assert "--achromatic: class 0 is not one of HoneyBee's receptor classes 1..3" in _error(capsys, [IN] + BEE + ["--achromatic", "1+0:0.1"])
    assert "--achromatic: CLASSES:E" in _error(capsys, [IN] + DOG + ["--achromatic", "LM:0.1"])
    assert "--achromatic: CLASSES:E" in _error(capsys, [IN] + DOG + ["--achromatic", "1"])
    assert "achromatic weber must be a number from 0.01 to 1" in _error(capsys, [IN] + DOG + ["--achromatic", "1:0.001"])
    assert "each once" in _error(capsys, [IN] + DOG + ["--achromatic", "1+1:0.1"])
    for bad in ("0", "9", "-1"):
        assert "--step must be 1..8" in _error(capsys, [IN] + DOG + [f"--step={bad}"])
    assert "HoneyBee has no acuity blur" in _error(capsys, [IN] + BEE + ["--acuity", "species"])
    assert "Rat has no acuity blur: its rendering ends with a gain per image row" in _error(capsys, [IN, "--observer", "Rat", "--weber", "0.1,0.1", "--acuity", "species"])
    assert "Sheep has no single acuity" in _error(capsys, [IN, "--observer", "Sheep", "--weber", "0.1,0.1", "--acuity", "species"])
    for bad in ("0.19", "4.07", "nan", "0"):
        assert "acuity must be a finite number of pixels from 0.2 to 4" in _error(capsys, [IN] + DOG + [f"--acuity={bad}"]), bad
    assert "--acuity: a number of pixels, or `species`" in _error(capsys, [IN] + DOG + ["--acuity", "Dog"])
    for bad in ("0", "17"):
        assert "--batch must be 1..16" in _error(capsys, [IN] + DOG + ["--batch", bad])
    for bad in ("0", "9"):
        assert "--depth must be 1..8" in _error(capsys, [IN] + DOG + ["--depth", bad])
    assert "--gain / --threshold: gain must be above 0" in _error(capsys, [IN, "o.npy"] + DOG + ["--gain", "0"])
    assert "--gain / --threshold: threshold must be finite" in _error(capsys, [IN] + DOG + ["--threshold", "-1"])
    for flag, v in (("--mode", "plain"), ("--gain", "4"), ("--out-pix-fmt", "nv12")):
        assert f"{flag} shapes the video that OUT names" in _error(capsys, [IN] + DOG + [flag, v])
    assert "--pix-fmt and --size go together" in _error(capsys, ["clip.yuv"] + DOG + ["--pix-fmt", "nv12"])
    assert "--scale 128x96 enlarges the 64x48 source" in _error(capsys, [IN] + DOG + ["--scale", "128x96"])
    assert "invalid choice" in _error(capsys, [IN] + DOG + ["--channel", "luminance"])


def test_command_summary_csv_and_launch(monkeypatch, capsys, tmp_path):
    from animal_vision_amd import edges
    from animal_vision_amd.deltae import CSV_HEADER, format_row
    from animal_vision_amd.metrics import DeltaE, observer_for

    h = np.zeros(256, np.int64)
    h[0], h[4] = 14, 10
    rec = DeltaE(h, 24.0, 2.25, 5, 2, 10)
    monkeypatch.setattr(edges, "stream_records", lambda args, info, fmt=None: iter([(None, rec)]))
    assert edges.main([IN] + DOG + ["--achromatic", "1:0.1", "--channel", "either", "--acuity", "species"]) == 0
    cap = capsys.readouterr()
    assert ("edges: 1 frames, mean RNL edges (Dog, weber 0.05,0.05, floor 0.001, achromatic 1:0.1, channel either, acuity 3.5 px, step 1) 1.000000, "
            "largest 2.250000 (frame 0, pixel x 5 y 2), 10 pixels beyond 1") in cap.err
    assert cap.out == CSV_HEADER + "\n" + format_row(0, rec) + "\n" and CSV_HEADER == "frame,de_mean,de_p50,de_p95,de_max,x,y,beyond"
    csv = tmp_path / "f.csv"
    assert edges.main([IN] + DOG + ["--csv", str(csv)]) == 0
    cap = capsys.readouterr()
    assert cap.out == "" and csv.read_text() == CSV_HEADER + "\n" + format_row(0, rec) + "\n" and "RNL edges (Dog, weber 0.05,0.05, floor 0.001, step 1)" in cap.err


# ------------------------------------------------------------------------------------------------ the Python entries
def test_metrics_refuse_bad_arguments_before_the_device(monkeypatch):
    from animal_vision_amd import metrics

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    dog = metrics.observer_for("Dog", (0.05, 0.05))
    bee = metrics.observer_for("HoneyBee", (0.13, 0.06, 0.12))
    f = np.zeros((12, 14, 3), np.uint8)
    entries = (metrics.receptor_edges, metrics.receptor_edges_map, metrics.receptor_edges_values)
    bad = [(dict(acuity=0.1), "acuity must be a finite number of pixels"), (dict(acuity=float("nan")), "acuity must be a finite number of pixels"),
           (dict(acuity="dog"), "acuity must be None, a number of pixels or 'species'"), (dict(step=0), "step must be a whole number of pixels from 1 to 8"),
           (dict(step=9), "step must be"), (dict(step=1.5), "step must be"), (dict(channel="either"), "channel 'either' needs achromatic"),
           (dict(channel="achromatic"), "channel 'achromatic' needs achromatic"), (dict(channel="luma"), "channel must be one of chromatic, achromatic, either"),
           (dict(achromatic=((3,), 0.1)), "achromatic class 3 is not one of Dog's receptor classes 1..2"),
           (dict(achromatic=((0,), 0.1)), "achromatic class 0 is not one of"), (dict(achromatic=((), 0.1)), "at least one receptor class"),
           (dict(achromatic=((1, 1), 0.1)), "each once"), (dict(achromatic=((1,), 0.001)), "achromatic weber must be a number from 0.01 to 1"),
           (dict(achromatic=((1,), 2.0)), "achromatic weber"), (dict(achromatic=0.1), r"achromatic must be \(classes, weber\)"),
           (dict(achromatic=((1.0,), 0.1)), "achromatic class 1.0 is not one of")]
    for kw, words in bad:
        for fn in entries:
            with pytest.raises(ValueError, match=words):
                fn(f, dog, **kw)
    with pytest.raises(ValueError, match="HoneyBee has no acuity blur"):
        metrics.receptor_edges(f, bee, acuity="species")
    with pytest.raises(ValueError, match="threshold must be finite"):
        metrics.receptor_edges(f, dog, threshold=-1)
    with pytest.raises(ValueError, match="gain must be above 0"):
        metrics.receptor_edges_map(f, dog, gain=0)
    with pytest.raises(ValueError, match="mode must be one of"):
        metrics.receptor_edges_map(f, dog, mode="side")
    with pytest.raises(ValueError, match="observer must be an Observer"):
        metrics.receptor_edges(f, "Dog")
    for shape, dtype in (((12, 14), np.uint8), ((12, 14, 4), np.uint8), ((0, 14, 3), np.uint8), ((12, 14, 3), np.float32)):
        with pytest.raises(ValueError, match="uint8|expected H x W x 3"):
            metrics.receptor_edges(np.zeros(shape, dtype), dog)
    with pytest.raises(AssertionError, match="the device was asked for"):  # good arguments do reach the device
        metrics.receptor_edges_values(f, dog, achromatic=((1,), 0.1), acuity="species", step=8)

    class Buf:
        ptr, nbytes = 0, 12 * 14 * 3

    class Rec:
        ptr, nbytes = 0, metrics.DELTA_E_RECORD_BYTES

    for kw, words in bad:
        with pytest.raises(ValueError, match=words):
            metrics.receptor_edges_launch(None, Buf(), 1, 12, 14, None, Rec(), observer=dog, **kw)
    with pytest.raises(ValueError, match="need 1008 bytes"):
        metrics.receptor_edges_launch(None, Buf(), 2, 12, 14, None, Rec(), observer=dog)
    with pytest.raises(ValueError, match="records need"):
        metrics.receptor_edges_launch(None, Buf(), 1, 12, 14, None, Buf(), observer=dog)
    with pytest.raises(ValueError, match="n_frames must be 1..16"):
        metrics.receptor_edges_launch(None, Buf(), 17, 12, 14, None, Rec(), observer=dog)


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib

    fn = _lib.lib.avx_receptor_edges_u8
    assert "avx_receptor_edges_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 17
    assert fn.argtypes[5] is ctypes.POINTER(_lib.ReceptorDesc) and fn.argtypes[6] is ctypes.POINTER(_lib.LuminanceDesc)
    assert fn.argtypes[8] is ctypes.c_double and fn.argtypes[11] is ctypes.c_float and fn.argtypes[12] is ctypes.c_float
    assert fn(None, None, 1, 16, 16, None, None, 0, 0.0, 1, 0, 10.0, 1.0, None, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context is refused first
    assert _lib.lib.avx_abi_version() == 1 and ctypes.sizeof(_lib.ReceptorDesc) == 144  # the observer's descriptor is not touched
    assert [(n, t) for n, t in _lib.LuminanceDesc._fields_] == [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("row", ctypes.c_double * 3),
                                                                ("weber", ctypes.c_double)]
    assert ctypes.sizeof(_lib.LuminanceDesc) == 40 and _lib.LuminanceDesc.row.offset == 8 and _lib.LuminanceDesc.weber.offset == 32
    assert _lib.AVX_EDGES_CHANNELS == {"chromatic": 0, "achromatic": 1, "either": 2}
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert ("int avx_receptor_edges_u8(avx_ctx* ctx, const uint8_t* hwc, int n_frames, int H, int W, const avx_receptor_desc* obs, const avx_luminance_desc* lum,\n"
            "                          int channel, double sigma, int step, int mode, float gain, float threshold, uint8_t* map_out, avx_delta_e_rec* rec_dev,\n"
            "                          float* ds_out, void* stream);") in hdr
    assert ("typedef struct avx_luminance_desc {\n    uint32_t struct_size;  /* sizeof(avx_luminance_desc) */\n    uint32_t reserved;     /* not read */\n"
            "    double row[3];         /* the sensitivity on linear RGB */\n    double weber;          /* e_L */\n} avx_luminance_desc;") in hdr
    assert "enum avx_edges_channel { AVX_EDGES_CHROMATIC = 0, AVX_EDGES_ACHROMATIC = 1, AVX_EDGES_EITHER = 2 };" in hdr
    assert "#define AVX_ABI_VERSION 1" in hdr and "v(p, n) = v(n, p) bit for bit" in hdr
    csrc = os.path.join(ROOT, "animal-vision_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "receptor_edges.hip" in mk and "receptor_common.h" in mk
    # one copy of the quadratic form: all three kernels take it from the shared header
    for name in ("receptor.hip", "receptor_acuity.hip", "receptor_edges.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "receptor_common.h"' in src and "Rnl<K>" in src and "pair_class" not in src, name
    src = open(os.path.join(csrc, "receptor_edges.hip")).read()
    assert "from_contrasts(" in src and "rnl_catch(" in src and "de_record_share(" in src and "de_px_panels(" in src and "atomicAdd(" not in src
