"""No GPU: the host side of the colour difference maps and the deltae command -- the yardstick of tests/_deltae_ref.py
against Sharma's published pairs and against itself, the record's percentile, the CSV line, the command's parser with its defaults and
its refusals by message, the command's bookkeeping with the device loop stubbed, the argument checks that need no device, the decode
table of the kernel, and the exported symbol with its prototype."""
import ctypes
import os
import re

import numpy as np
import pytest

import _deltae_ref as E
from animal_vision_amd import deltae as _deltae_module  # noqa: F401  (the feature: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_reproduces_sharmas_pairs():
    for l1, l2, want in (((50, 2.6772, -79.7751), (50, 0, -82.7485), 2.0425), ((50, 3.1571, -77.2803), (50, 0, -82.7485), 2.8615),
                         ((50, 2.8361, -74.0200), (50, 0, -82.7485), 3.4412)):
        got = float(E.ciede2000(np.array(l1, np.float64), np.array(l2, np.float64)))
        assert round(got, 4) == want, (l1, l2, got)


def test_yardstick_on_code_pairs():
    for x, y, want in (((0, 0, 0), (255, 255, 255), 100.0), ((0, 0, 255), (255, 255, 0), 103.4270), ((0, 255, 0), (255, 0, 255), 111.4143)):
        got = float(E.delta_e(np.array(x, np.uint8), np.array(y, np.uint8)))
        assert abs(got - want) <= 1e-4, (x, y, got)
    grey = np.repeat(np.arange(1, 255, dtype=np.uint8)[:, None], 3, axis=1)
    step = grey.copy()
    step[:, 1] += 1
    de = E.delta_e(grey, step)  # a one-code step in G on a grey
    assert round(float(de.min()), 2) == 0.67 and round(float(de.max()), 2) == 1.23, (de.min(), de.max())
    assert float(E.delta_e(np.array([7, 8, 9], np.uint8), np.array([7, 8, 9], np.uint8))) == 0.0
    assert np.array_equal(E.lab(np.array([255, 255, 255], np.uint8)).round(9), [100.0, 0.0, 0.0])


def test_yardstick_is_symmetric():
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 256, (20000, 3), dtype=np.uint8), rng.integers(0, 256, (20000, 3), dtype=np.uint8)
    ab, ba = E.delta_e(a, b), E.delta_e(b, a)
    assert np.abs(ab - ba).max() <= 1e-12 and ab.max() > 100.0 and (ab >= 0).all()
    for _, x, y in E.frames(29, 37, 3):
        assert np.abs(E.delta_e(x, y) - E.delta_e(y, x)).max() <= 1e-12


def test_every_grey_is_exactly_achromatic_in_float32():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    lab32 = E.lab(grey, np.float32)
    assert lab32.dtype == np.float32 and (lab32[:, 1] == 0).all() and (lab32[:, 2] == 0).all()
    assert (np.diff(lab32[:, 0]) > 0).all() and lab32[0, 0] == 0 and abs(float(lab32[255, 0]) - 100.0) < 1e-4
    lab64 = E.lab(grey)
    assert (lab64[:, 1:] == 0).all()
    # a grey against a colour has no hue of its own: the colour's hue is the mean hue
    h1, h2, c1, c2 = E.hues(E.lab(grey[128]), E.lab(np.array([0, 0, 255], np.uint8)))
    assert h1 == 0 and c1 == 0 and c2 > 100 and 300 < h2 < 310


def test_percentile_on_hand_made_histograms():
    from animal_vision_amd.metrics import DeltaE

    h = np.zeros(256, np.int64)
    h[0], h[3], h[9] = 50, 45, 5  # 100 pixels
    r = DeltaE(h, 123.0, 4.9, 1, 2, 5)
    assert r.pixels == 100 and r.mean == 1.23
    assert r.percentile(0.5) == 0.5 and r.percentile(0.51) == 2.0 and r.percentile(0.95) == 2.0 and r.percentile(0.951) == 5.0 and r.percentile(1.0) == 5.0
    assert r.percentile(0.001) == 0.5
    for q in (0.5, 0.51, 0.95, 0.951, 1.0, 0.001):
        assert r.percentile(q) == E.percentile(h, 4.9, q), q
    h[9], h[255] = 0, 5  # the open last bin: its upper edge is the largest value
    r = DeltaE(h, 1000.0, 131.25, 0, 0, 5)
    assert r.percentile(0.95) == 2.0 and r.percentile(0.96) == 131.25 == E.percentile(h, 131.25, 0.96) and r.percentile(1.0) == 131.25
    h[:] = 0
    h[254] = 7
    assert DeltaE(h, 0.0, 127.4, 0, 0, 7).percentile(0.5) == 127.5  # the last closed bin still answers with its edge
    with pytest.raises(ValueError, match="above 0 and at most 1"):
        r.percentile(0.0)
    with pytest.raises(ValueError, match="256 bins"):
        DeltaE(np.zeros(255), 0, 0, 0, 0, 0)
    assert DeltaE(h, 1.0, 2.0, 3, 4, 5) == DeltaE(h, 1.0, 2.0, 3, 4, 5) != DeltaE(h, 1.0, 2.0, 3, 4, 6)


def test_reference_record_and_quantiser_on_hand_made_values():
    v = np.array([[0.0, 0.49, 0.5], [3.2, 130.0, 3.2]], np.float32)
    r = E.record(v, 1.0)
    assert r["hist"][0] == 2 and r["hist"][1] == 1 and r["hist"][6] == 2 and r["hist"][255] == 1 and r["hist"].sum() == 6
    assert (r["max_de"], r["max_x"], r["max_y"], r["beyond"]) == (130.0, 1, 1, 3)
    v[1, 1] = 3.2
    assert (E.record(v, 3.2)["max_x"], E.record(v, 3.2)["max_y"], E.record(v, 3.2)["beyond"]) == (0, 1, 0)  # the first among equals; > T, not >=
    assert E.record(np.zeros((2, 2), np.float32), 0.0)["max_x"] == 0
    assert E.quantise(np.array([0.0, 1.0, 1.04, 1.06, 26.5, 1e3], np.float32), 10.0, 1.0, "heat").tolist() == [0, 0, 0, 1, 255, 255]
    assert E.quantise(np.array([0.0, 0.04, 0.06, 25.5], np.float32), 10.0, 1.0, "plain").tolist() == [0, 0, 1, 255]
    a = np.array([[10, 20, 30], [200, 100, 50]], np.uint8)
    m = E.de_map(np.array([1.0, 2.0], np.float32), a, 10.0, 1.0, "heat")
    g0 = ((77 * 10 + 150 * 20 + 29 * 30 + 128) >> 8) >> 2
    assert m.tolist() == [[g0] * 3, [30, 0, 0]]
    assert E.de_map(np.array([0.0, 2.0], np.float32), a, 10.0, 1.0, "plain").tolist() == [[0, 0, 0], [60, 0, 0]]


def test_csv_formatting():
    from animal_vision_amd import deltae
    from animal_vision_amd.metrics import DeltaE

    h = np.zeros(256, np.int64)
    h[0], h[3], h[9] = 50, 45, 5
    assert deltae.CSV_HEADER == "frame,de_mean,de_p50,de_p95,de_max,x,y,beyond"
    assert deltae.format_row(7, DeltaE(h, 123.0, 4.75, 11, 2, 5)) == "7,1.230000,0.500000,2.000000,4.750000,11,2,5"
    h[:] = 0
    h[0] = 12
    assert deltae.format_row(0, DeltaE(h, 0.0, 0.0, 0, 0, 0)) == "0,0.000000,0.500000,0.500000,0.000000,0,0,0"


# ------------------------------------------------------------------------------------------------ the parser
def _error(capsys, argv):
    from animal_vision_amd import deltae

    with pytest.raises(SystemExit) as e:
        deltae.parse_args(argv)
    assert e.value.code == 2, argv
    return capsys.readouterr().err


def test_parser_defaults_and_shared_options():
    from animal_vision_amd import deltae

    a = deltae.parse_args(["a.y4m", "b.npy"])
    assert (a.a, a.b, a.out, a.mode, a.gain, a.threshold, a.layout) == ("a.y4m", "b.npy", None, "heat", 10.0, 1.0, "map")
    assert (a.batch, a.depth, a.csv, a.shortest, a.matrix, a.scale, a.max_mean, a.max_p95, a.max_de) == (8, 2, None, False, "bt601", None, None, None, None)
    assert deltae.sink_format(a) is None
    a = deltae.parse_args(["a.y4m", "b.npy", "out.y4m"])
    assert (a.out, a.mode, a.gain, a.threshold, a.layout, a.depth) == ("out.y4m", "heat", 10.0, 1.0, "map", 2) and deltae.sink_format(a) == "i420"
    a = deltae.parse_args(["a.yuv", "b.yuv", "-", "--pix-fmt", "nv12", "--size", "64x48", "--matrix", "bt709", "--range", "full", "--scale", "32x24",
                           "--batch", "16", "--depth", "8", "--mode", "plain", "--gain", "0.5", "--threshold", "0", "--layout", "side", "--csv", "w.csv",
                           "--shortest", "--max-mean", "1", "--max-p95", "2.5", "--max-de", "30"])
    assert (a.pix_fmt, a.size, a.matrix, a.range, a.scale, a.batch, a.depth) == ("nv12", (64, 48), "bt709", "full", (32, 24), 16, 8)
    assert (a.mode, a.gain, a.threshold, a.layout, a.csv, a.shortest) == ("plain", 0.5, 0.0, "side", "w.csv", True)
    assert (a.max_mean, a.max_p95, a.max_de) == (1.0, 2.5, 30.0)
    assert deltae.sink_format(a) == "nv12"  # "-" with a raw input: the input's format, as in `video`
    assert deltae.sink_format(deltae.parse_args(["a", "b", "o.npy"])) is None and deltae.sink_format(deltae.parse_args(["a", "b", "frames/"])) is None
    assert deltae.sink_format(deltae.parse_args(["a", "b", "o.yuv", "--out-pix-fmt", "yuv444p"])) == "yuv444p"
    a = deltae.parse_args(["a.yuv", "b.yuv", "--pix-fmt", "p010le", "--size", "64x48", "--transfer", "pq", "--tonemap", "clip", "--threshold", "2.5"])
    assert (a.transfer, a.tonemap, a.peak_nits, a.sdr_white, a.threshold, a.out) == ("pq", "clip", 1000.0, 203.0, 2.5, None)


def test_parser_refusals_by_message(capsys):
    assert "A and B cannot both be stdin" in _error(capsys, ["-", "-"])
    assert "gain must be above 0 and at most 255" in _error(capsys, ["a", "b", "o", "--gain", "0"])
    assert "gain must be above 0 and at most 255" in _error(capsys, ["a", "b", "o", "--gain", "255.5"])
    assert "gain must be above 0 and at most 255" in _error(capsys, ["a", "b", "o", "--gain", "nan"])
    assert "gain must be above 0 and at most 255" in _error(capsys, ["a", "b", "o", "--gain", "inf"])
    assert "threshold must be finite and at least 0" in _error(capsys, ["a", "b", "--threshold", "-0.5"])
    assert "threshold must be finite and at least 0" in _error(capsys, ["a", "b", "o", "--threshold", "inf"])
    assert "threshold must be finite and at least 0" in _error(capsys, ["a", "b", "--threshold", "nan"])
    assert "--depth must be 1..8" in _error(capsys, ["a", "b", "o", "--depth", "0"])
    assert "--depth must be 1..8" in _error(capsys, ["a", "b", "o", "--depth", "9"])
    assert "--max-p95 must be finite and at least 0" in _error(capsys, ["a", "b", "--max-p95", "-1"])
    assert "--max-mean must be finite and at least 0" in _error(capsys, ["a", "b", "--max-mean", "nan"])
    assert "--max-de must be finite and at least 0" in _error(capsys, ["a", "b", "--max-de", "inf"])
    assert "--pix-fmt and --size go together" in _error(capsys, ["a", "b", "--pix-fmt", "nv12"])
    assert "--tonemap needs --transfer" in _error(capsys, ["a", "b", "o", "--tonemap", "clip"])
    assert "enlarges" in _error(capsys, ["synthetic:32x24:2", "synthetic:64x48:2", "--scale", "64x48"])
    assert "enlarges" in _error(capsys, ["a.npy", "synthetic:32x24:2", "--scale", "64x48"])
    for bad in (["a"], ["a", "b", "o", "p"], ["a", "b", "o", "--species", "Dog"], ["a", "b", "o", "--mode", "abs"], ["a", "b", "o", "--mode", "ssim"],
                ["a", "b", "o", "--layout", "top"], ["a", "b", "--batch", "17"], ["a", "b", "--max-abs", "1"], ["a", "b", "--min-ssim", "0.9"]):
        _error(capsys, bad)


def test_without_out_the_output_only_options_are_refused_by_name(capsys):
    for flag, value in (("--out-pix-fmt", "nv12"), ("--out-matrix", "bt709"), ("--depth", "2"), ("--mode", "heat"), ("--gain", "10"), ("--layout", "map")):
        err = _error(capsys, ["a.npy", "b.npy", flag, value])
        assert f"{flag} shapes the video that OUT names: without OUT deltae writes none" in err, flag
    from animal_vision_amd import deltae

    a = deltae.parse_args(["a.npy", "b.npy", "--threshold", "2", "--csv", "x.csv", "--batch", "4", "--shortest"])  # these belong to the statistics
    assert (a.threshold, a.csv, a.batch) == (2.0, "x.csv", 4)


# ------------------------------------------------------------------------------------------------ the command, the device loop stubbed
def _records():
    from animal_vision_amd.metrics import DeltaE

    h0 = np.zeros(256, np.int64)
    h0[0] = 24
    h1 = np.zeros(256, np.int64)
    h1[0], h1[4], h1[20] = 12, 10, 2
    return [DeltaE(h0, 0.0, 0.0, 0, 0, 0), DeltaE(h1, 48.0, 10.25, 5, 2, 12), DeltaE(h1, 36.0, 10.25, 1, 1, 12)]


def _run(monkeypatch, capsys, items, argv, longer=None, hw=(4, 6)):
    from animal_vision_amd import deltae

    def stub(args, info, fmt=None):
        assert fmt is None
        info["hw"] = hw
        if longer:
            info["longer"] = longer
        yield from items

    monkeypatch.setattr(deltae, "stream_records", stub)
    status = deltae.main(argv)
    cap = capsys.readouterr()
    return status, cap.out, cap.err


def test_command_bookkeeping(monkeypatch, capsys, tmp_path):
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (3, 4, 6, 3), dtype=np.uint8)
    recs = _records()
    rows = ["frame,de_mean,de_p50,de_p95,de_max,x,y,beyond", "0,0.000000,0.500000,0.500000,0.000000,0,0,0", "1,2.000000,0.500000,10.500000,10.250000,5,2,12",
            "2,1.500000,0.500000,10.500000,10.250000,1,1,12"]
    out, csv = tmp_path / "o.npy", tmp_path / "w.csv"
    status, stdout, err = _run(monkeypatch, capsys, list(zip(frames, recs)), ["a.npy", "b.npy", str(out), "--csv", str(csv)])
    assert status == 0 and stdout == ""  # with OUT the lines never go to stdout
    assert np.array_equal(np.load(out), frames)
    assert csv.read_text().splitlines() == rows
    # the summary: frames, the mean of the frame means, the largest dE with the first frame that attains it, pixels beyond T, fps
    assert "deltae: 3 frames, mean dE 1.166667, largest dE 10.250000 (frame 1, pixel x 5 y 2), 24 pixels beyond 1," in err and "fps" in err
    # without OUT: the same lines on stdout, or in --csv
    none = [(None, r) for r in recs]
    status, stdout, err = _run(monkeypatch, capsys, none, ["a.npy", "b.npy"])
    assert status == 0 and stdout.splitlines() == rows and "deltae: 3 frames" in err
    status, stdout, err = _run(monkeypatch, capsys, none, ["a.npy", "b.npy", "--csv", str(csv), "--threshold", "3"])
    assert status == 0 and stdout == "" and csv.read_text().splitlines() == rows and "24 pixels beyond 3," in err
    # lengths
    status, stdout, err = _run(monkeypatch, capsys, none[:1], ["a.npy", "b.npy"], longer="B")
    assert status == 2 and "B has more frames than the other input: compared the first 1" in err and "largest dE 0.000000, 0 pixels beyond 1" in err
    status, stdout, err = _run(monkeypatch, capsys, none[:1], ["a.npy", "b.npy", "--shortest"], longer="A")
    assert status == 0 and "more frames" not in err
    status, stdout, err = _run(monkeypatch, capsys, [], ["a.npy", "b.npy"])
    assert status == 0 and stdout.splitlines() == rows[:1] and "deltae: 0 frames, mean dE nan" in err
    # the limits: status 1, the first frame that breaks one is named
    for argv, line in ((["--max-mean", "1.75"], "deltae: frame 1: mean dE 2.000000 is above --max-mean 1.75"),
                       (["--max-mean", "1.25"], "deltae: frame 1: mean dE 2.000000 is above --max-mean 1.25"),
                       (["--max-p95", "10"], "deltae: frame 1: 95th percentile dE 10.500000 is above --max-p95 10"),
                       (["--max-de", "10"], "deltae: frame 1: largest dE 10.250000 (pixel x 5 y 2) is above --max-de 10")):
        status, stdout, err = _run(monkeypatch, capsys, none, ["a.npy", "b.npy"] + argv)
        assert status == 1 and line in err and len(stdout.splitlines()) == 4, argv  # every line is still written
    status, _, err = _run(monkeypatch, capsys, none, ["a.npy", "b.npy", "--max-mean", "2", "--max-p95", "10.5", "--max-de", "10.25"])
    assert status == 0 and "frame 1:" not in err  # a limit is broken above it, not at it
    status, _, err = _run(monkeypatch, capsys, none[1:], ["a.npy", "b.npy", "--max-de", "10"], longer="A")
    assert status == 1 and "more frames" in err and "deltae: frame 0: largest dE" in err  # a broken limit outranks the length
    pngs = tmp_path / "pngs"
    status, stdout, err = _run(monkeypatch, capsys, list(zip(frames, recs)), ["a.npy", "b.npy", str(pngs)])
    assert status == 0 and sorted(os.listdir(pngs)) == [f"frame_{i:06d}.png" for i in range(3)]


# ------------------------------------------------------------------------------------------------ metrics.delta_e* without a device
def test_delta_e_refuses_bad_arguments_before_the_device(monkeypatch):
    from animal_vision_amd import metrics

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    a = np.zeros((12, 14, 3), np.uint8)
    with pytest.raises(ValueError, match=r"\(12, 14, 3\).*\(12, 15, 3\)"):
        metrics.delta_e_map(a, np.zeros((12, 15, 3), np.uint8))
    with pytest.raises(ValueError, match=r"uint8.*float32"):
        metrics.delta_e(a, a.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        metrics.delta_e_values(a.astype(np.uint16), a)
    for kw, msg in ((dict(mode="abs"), "mode must be one of heat, plain"), (dict(layout="top"), "layout must be one of map, side"),
                    (dict(threshold=-1.0), "threshold must be finite and at least 0"), (dict(threshold=float("nan")), "threshold must be finite"),
                    (dict(threshold="1"), "threshold must be finite"), (dict(gain=0), "gain must be above 0 and at most 255"),
                    (dict(gain=255.5), "gain must be above 0"), (dict(gain=float("inf")), "gain must be above 0"), (dict(gain=True), "gain must be above 0")):
        with pytest.raises(ValueError, match=msg):
            metrics.delta_e_map(a, a, **kw)
    with pytest.raises(ValueError, match="threshold must be finite and at least 0"):
        metrics.delta_e(a, a, threshold=-1)
    for call in (lambda: metrics.delta_e(a, a), lambda: metrics.delta_e_values(a, a),
                 lambda: metrics.delta_e_map(a, a, mode="plain", gain=255, threshold=0, layout="side")):
        with pytest.raises(AssertionError, match="the device was asked for"):
            call()
    assert metrics.check_delta_e_options() == (10.0, 1.0) and metrics.check_delta_e_options("plain", 0.25, 0, "side") == (0.25, 0.0)
    assert metrics.DELTA_E_MODES == ("heat", "plain") and metrics.DELTA_E_LAYOUTS == ("map", "side")

    class Buf:
        ptr, nbytes = 0, 12 * 14 * 3

    class Rec:
        ptr, nbytes = 0, metrics.DELTA_E_RECORD_BYTES

    with pytest.raises(ValueError, match="side frames need"):
        metrics.delta_e_launch(None, Buf(), Buf(), 1, 12, 14, Buf(), Rec(), layout="side")  # the output holds one panel, not three
    with pytest.raises(ValueError, match="records need"):
        metrics.delta_e_launch(None, Buf(), Buf(), 1, 12, 14, None, Buf())
    with pytest.raises(ValueError, match="the values of 1 frames need"):
        metrics.delta_e_launch(None, Buf(), Buf(), 1, 12, 14, None, Rec(), d_float=Buf())  # 3 bytes a pixel, not 4
    with pytest.raises(ValueError):
        metrics.delta_e_launch(None, Buf(), Buf(), 17, 12, 14, None, Rec())


# ------------------------------------------------------------------------------------------------ the table and the symbol
def test_decode_table_is_the_formula_rounded_once():
    src = open(os.path.join(ROOT, "animal-vision_amd", "csrc", "lab_tables.h")).read()
    body = src[src.index("kLabDecodeBits[256]"):]
    bits = np.array([int(m, 16) for m in re.findall(r"0x([0-9a-f]{8})u", body)], np.uint32)
    assert bits.shape == (256,)
    assert np.array_equal(bits.view(np.float32), E.decode_table().astype(np.float32))
    # not the decode table of the species kernels: that one holds the reference's float32 arithmetic and differs in most entries
    other = np.load(os.path.join(ROOT, "tests", "golden", "srgb_tables.npz"))["decode_lut"]
    assert (other != bits.view(np.float32)).sum() > 100 and np.abs(other - bits.view(np.float32)).max() < 2e-7


def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib, metrics

    fn = _lib.lib.avx_delta_e_u8
    assert "avx_delta_e_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[7] is ctypes.c_float and fn.argtypes[8] is ctypes.c_float
    assert fn(None, None, None, 1, 16, 16, 0, 10.0, 1.0, 0, None, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context is refused first
    assert ctypes.sizeof(_lib.DeltaERecord) == 1048 == metrics.DELTA_E_RECORD_BYTES
    assert [f[0] for f in _lib.DeltaERecord._fields_] == ["hist", "sum", "max_de", "max_x", "max_y", "beyond"]
    assert (_lib.DeltaERecord.hist.offset, _lib.DeltaERecord.sum.offset, _lib.DeltaERecord.max_de.offset, _lib.DeltaERecord.beyond.offset) == (0, 1024, 1032, 1044)
    assert _lib.AVX_DELTA_E_MODES == {"heat": 0, "plain": 1} and _lib.AVX_DELTA_E_LAYOUTS == {"map": 0, "side": 1}
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert ("int avx_delta_e_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, float threshold,\n"
            "                   int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream);") in hdr
    assert "enum avx_delta_e_mode { AVX_DELTA_E_HEAT = 0, AVX_DELTA_E_PLAIN = 1 };" in hdr
    assert "enum avx_delta_e_layout { AVX_DELTA_E_MAP = 0, AVX_DELTA_E_SIDE = 1 };" in hdr
    assert "} avx_delta_e_rec;" in hdr and "#define AVX_ABI_VERSION 1" in hdr
    assert "delta_e.hip" in open(os.path.join(ROOT, "animal-vision_amd", "csrc", "Makefile")).read()
    # the quantiser of the map names its roundings: the multiply and the add are separate operations
    src = open(os.path.join(ROOT, "animal-vision_amd", "csrc", "delta_e.hip")).read()
    assert "__fmul_rn(" in src and "__fadd_rn(" in src
    # diff's enums are untouched
    assert _lib.AVX_DIFF_MODES == {"abs": 0, "heat": 1, "ssim": 2}
