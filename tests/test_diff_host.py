"""No GPU: the host side of the difference maps and the diff command -- the yardstick of tests/_diff_ref.py agrees with
itself and with _metrics_ref, the command's parser, its defaults and its refusals by message, the command's bookkeeping with the device
loop stubbed, the argument checks of metrics.diff_map that need no device, and the exported symbol with its prototype."""
import ctypes
import os

import numpy as np
import pytest

import _diff_ref as D
import _metrics_ref as R
from animal_vision_amd import diff as _diff_module  # noqa: F401  (the feature: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the yardstick
def test_palette_is_injective_and_sums_to_3v():
    v = np.arange(256)
    p = D.pal(v).astype(np.int64)
    assert p.shape == (256, 3) and (p.sum(axis=1) == 3 * v).all()
    assert len({tuple(row) for row in p}) == 256
    assert tuple(p[0]) == (0, 0, 0) and tuple(p[85]) == (255, 0, 0) and tuple(p[170]) == (255, 255, 0) and tuple(p[255]) == (255, 255, 255)
    assert (np.diff(p, axis=0) >= 0).all()  # black - red - yellow - white, never back


def test_reference_maps_on_hand_made_pixels():
    a = np.array([[[10, 20, 30], [200, 100, 50], [0, 0, 0], [255, 255, 255]]], np.uint8)
    b = np.array([[[10, 21, 30], [190, 100, 58], [0, 0, 0], [0, 255, 255]]], np.uint8)
    assert D.abs_map(a, b, 32).tolist() == [[[0, 32, 0], [255, 0, 255], [0, 0, 0], [255, 0, 0]]]
    h = D.heat_map(a, b, 32, 1)
    g0, g2 = ((77 * 10 + 150 * 20 + 29 * 30 + 128) >> 8) >> 2, 0
    assert h[0, 0].tolist() == [g0] * 3 and h[0, 2].tolist() == [g2] * 3                  # d = 1 and d = 0: within K = 1
    assert h[0, 1].tolist() == D.pal(255)[()].tolist() and h[0, 3].tolist() == [255] * 3  # 32 * 9 and 32 * 254 saturate
    assert D.heat_map(a, b, 1, 0)[0, 0].tolist() == [3, 0, 0]                             # K = 0: d = 1 is coloured, v = 1
    assert D.record(a, b, 1) == (255, 3, 0, 2) and D.record(a, b, 0) == (255, 3, 0, 3) and D.record(a, b, 254) == (255, 3, 0, 1)
    assert D.side(a, b, h).shape == (1, 12, 3)
    # the first pixel in raster order wins among equals
    x, y = np.zeros((4, 5, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)
    y[2, 1, 0] = y[1, 4, 2] = y[3, 0, 1] = 9
    assert D.record(x, y, 1) == (9, 4, 1, 3)


def test_reference_identical_frames_and_mean_of_the_map():
    for name, a, b in R.six_frames(23, 31):
        assert D.record(a, a, 0) == (0, 0, 0, 0), name
        assert (D.heat_map(a, a, 255, 0)[..., 0] == D.heat_map(a, a, 1, 254)[..., 1]).all()  # all grey: neither G nor K shows
        pos = D.ssim_positions(a, b)
        assert pos.shape == (13, 21, 3)
        for c, want in enumerate(R.ssim(a, b)):
            assert abs(pos[..., c].mean() - want) < 1e-12, (name, c)
        same = D.ssim_positions(a, a)
        assert (same == 1.0).all() and (D.ssim_mode_map(same, 16.0, 23, 31) == 0).all()
        m32 = D.map32(a, b)
        assert m32.dtype == np.float32 and m32.shape == pos.shape and np.abs(m32 - pos).max() < 1e-3, name
        assert (D.map32(a, a) == 1.0).all(), name


def test_reference_border_replication():
    pos = np.arange(3 * 4, dtype=np.int64).reshape(3, 4)  # 13 x 14 pixels
    px = D.replicate(pos, 13, 14)
    assert px.shape == (13, 14) and (px[:6, :6] == 0).all() and (px[7:, 8:] == 11).all() and px[6, 7] == pos[1, 2]
    assert (D.replicate(np.array([[7]]), 11, 11) == 7).all()


def test_fma32_rounds_once():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(20000).astype(np.float32) * np.float32(2.0) ** rng.integers(-12, 12, 20000).astype(np.float32) for _ in range(3))
    got = D.fma32(a, b, c)
    from fractions import Fraction

    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        e = abs(exact - Fraction(float(got[i])))
        assert e <= abs(exact - Fraction(float(lo))) and e <= abs(exact - Fraction(float(hi))), i


# ------------------------------------------------------------------------------------------------ the parser
def _error(capsys, argv):
    from animal_vision_amd import diff

    with pytest.raises(SystemExit) as e:
        diff.parse_args(argv)
    assert e.value.code == 2, argv
    return capsys.readouterr().err


def test_parser_defaults_and_shared_options():
    from animal_vision_amd import diff

    a = diff.parse_args(["a.y4m", "b.npy", "out.y4m"])
    assert (a.a, a.b, a.out, a.mode, a.gain, a.threshold, a.layout) == ("a.y4m", "b.npy", "out.y4m", "heat", 32.0, 1, "map")
    assert (a.batch, a.depth, a.csv, a.shortest, a.matrix, a.scale, a.out_pix_fmt) == (8, 2, None, False, "bt601", None, None)
    assert diff.sink_format(a) == "i420"
    assert diff.parse_args(["a", "b", "o", "--mode", "abs"]).gain == 32.0 and diff.parse_args(["a", "b", "o", "--mode", "ssim"]).gain == 4.0
    a = diff.parse_args(["a.yuv", "b.yuv", "-", "--pix-fmt", "nv12", "--size", "64x48", "--matrix", "bt709", "--range", "full", "--scale", "32x24",
                         "--batch", "16", "--depth", "8", "--mode", "ssim", "--gain", "0.5", "--threshold", "0", "--layout", "side", "--csv", "w.csv",
                         "--shortest"])
    assert (a.pix_fmt, a.size, a.matrix, a.range, a.scale, a.batch, a.depth) == ("nv12", (64, 48), "bt709", "full", (32, 24), 16, 8)
    assert (a.mode, a.gain, a.threshold, a.layout, a.csv, a.shortest) == ("ssim", 0.5, 0, "side", "w.csv", True)
    assert diff.sink_format(a) == "nv12"  # "-" with a raw input: the input's format, as in `video`
    assert diff.sink_format(diff.parse_args(["a", "b", "o.npy"])) is None and diff.sink_format(diff.parse_args(["a", "b", "frames/"])) is None
    assert diff.sink_format(diff.parse_args(["a", "b", "o.yuv", "--out-pix-fmt", "yuv444p"])) == "yuv444p"
    a = diff.parse_args(["a.yuv", "b.yuv", "o.y4m", "--pix-fmt", "p010le", "--size", "64x48", "--transfer", "pq", "--tonemap", "clip"])
    assert (a.transfer, a.tonemap, a.peak_nits, a.sdr_white) == ("pq", "clip", 1000.0, 203.0) and diff.sink_format(a) == "i420"
    # the help says what `beyond` counts
    assert "pixels, where compare's beyond1 counts samples" in " ".join(diff.build_parser().format_help().split())


def test_parser_refusals_by_message(capsys):
    assert "A and B cannot both be stdin" in _error(capsys, ["-", "-", "o.y4m"])
    assert "--mode heat multiplies code differences and takes an integer 1..255" in _error(capsys, ["a", "b", "o", "--gain", "2.5"])
    assert "--mode abs multiplies code differences" in _error(capsys, ["a", "b", "o", "--mode", "abs", "--gain", "0.5"])
    assert "integer 1..255" in _error(capsys, ["a", "b", "o", "--gain", "0"])
    assert "integer 1..255" in _error(capsys, ["a", "b", "o", "--mode", "abs", "--gain", "256"])
    assert "above 0 and at most 16" in _error(capsys, ["a", "b", "o", "--mode", "ssim", "--gain", "17"])
    assert "above 0 and at most 16" in _error(capsys, ["a", "b", "o", "--mode", "ssim", "--gain", "0"])
    assert "threshold must be an integer 0..254" in _error(capsys, ["a", "b", "o", "--threshold", "255"])
    assert "threshold must be an integer 0..254" in _error(capsys, ["a", "b", "o", "--threshold", "-1"])
    assert "--mode ssim needs frames of at least 11x11; these are 40x10" in _error(capsys, ["synthetic:40x10:2", "b.npy", "o", "--mode", "ssim"])
    assert "these are 10x40" in _error(capsys, ["a.npy", "synthetic:10x40:2", "o", "--mode", "ssim"])
    assert "these are 8x8" in _error(capsys, ["a.yuv", "b.yuv", "o", "--mode", "ssim", "--pix-fmt", "nv12", "--size", "64x48", "--scale", "8x8"])
    assert "--depth must be 1..8" in _error(capsys, ["a", "b", "o", "--depth", "0"])
    assert "--depth must be 1..8" in _error(capsys, ["a", "b", "o", "--depth", "9"])
    assert "--pix-fmt and --size go together" in _error(capsys, ["a", "b", "o", "--pix-fmt", "nv12"])
    assert "--tonemap needs --transfer" in _error(capsys, ["a", "b", "o", "--tonemap", "clip"])
    assert "enlarges" in _error(capsys, ["synthetic:32x24:2", "synthetic:64x48:2", "o", "--scale", "64x48"])
    for bad in (["a", "b"], ["a", "b", "o", "--species", "Dog"], ["a", "b", "o", "--mode", "psnr"], ["a", "b", "o", "--layout", "top"],
                ["a", "b", "o", "--batch", "17"], ["a", "b", "o", "--max-abs", "1"]):
        _error(capsys, bad)
    # a size the command line does not show is not judged here: the device loop refuses it when the input is open
    from animal_vision_amd import diff

    assert diff.parse_args(["a.npy", "b.npy", "o", "--mode", "ssim"]).mode == "ssim"


# ------------------------------------------------------------------------------------------------ the command, the device loop stubbed
def _run(monkeypatch, capsys, items, argv, longer=None, hw=(4, 6)):
    from animal_vision_amd import diff

    def stub(args, info, fmt=None):
        assert fmt is None
        info["hw"] = hw
        if longer:
            info["longer"] = longer
        yield from items

    monkeypatch.setattr(diff, "stream_maps", stub)
    status = diff.main(argv)
    cap = capsys.readouterr()
    return status, cap.out, cap.err


def test_command_bookkeeping(monkeypatch, capsys, tmp_path):
    from animal_vision_amd.metrics import DiffRecord

    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (3, 4, 6, 3), dtype=np.uint8)
    recs = [DiffRecord(0, 0, 0, 0), DiffRecord(7, 5, 2, 9), DiffRecord(7, 1, 1, 4)]
    out, csv = tmp_path / "o.npy", tmp_path / "w.csv"
    status, stdout, err = _run(monkeypatch, capsys, list(zip(frames, recs)), ["a.npy", "b.npy", str(out), "--csv", str(csv)])
    assert status == 0 and stdout == ""
    assert np.array_equal(np.load(out), frames)
    assert csv.read_text().splitlines() == ["frame,max_d,x,y,beyond", "0,0,0,0,0", "1,7,5,2,9", "2,7,1,1,4"]
    assert "diff: 3 frames, largest difference 7 (frame 1, pixel x 5 y 2), 13 pixels beyond 1," in err and "fps" in err  # the first frame that attains it
    status, stdout, err = _run(monkeypatch, capsys, list(zip(frames[:1], recs[:1])), ["a.npy", "b.npy", str(tmp_path / "p.npy"), "--threshold", "3"], longer="B")
    assert status == 2 and "B has more frames than the other input: compared the first 1" in err and "largest difference 0, 0 pixels beyond 3" in err
    status, stdout, err = _run(monkeypatch, capsys, list(zip(frames[:1], recs[:1])), ["a.npy", "b.npy", str(tmp_path / "q.npy"), "--shortest"], longer="A")
    assert status == 0 and "more frames" not in err
    pngs = tmp_path / "pngs"
    status, stdout, err = _run(monkeypatch, capsys, list(zip(frames, recs)), ["a.npy", "b.npy", str(pngs)])
    assert status == 0 and sorted(os.listdir(pngs)) == [f"frame_{i:06d}.png" for i in range(3)]


# ------------------------------------------------------------------------------------------------ metrics.diff_map without a device
def test_diff_map_refuses_bad_arguments_before_the_device(monkeypatch):
    from animal_vision_amd import metrics

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    a = np.zeros((12, 14, 3), np.uint8)
    with pytest.raises(ValueError, match=r"\(12, 14, 3\).*\(12, 15, 3\)"):
        metrics.diff_map(a, np.zeros((12, 15, 3), np.uint8))
    with pytest.raises(ValueError, match=r"uint8.*float32"):
        metrics.diff_map(a, a.astype(np.float32))
    for kw, msg in ((dict(mode="psnr"), "mode must be one of abs, heat, ssim"), (dict(layout="top"), "layout must be one of map, side"),
                    (dict(threshold=255), "threshold must be an integer 0..254"), (dict(threshold=1.5), "threshold must be an integer"),
                    (dict(gain=0), "gain of mode heat must be an integer 1..255"), (dict(gain=2.5), "integer 1..255"),
                    (dict(mode="abs", gain=256), "gain of mode abs"), (dict(mode="ssim", gain=16.5), "above 0 and at most 16"),
                    (dict(mode="ssim", gain=0.0), "above 0 and at most 16")):
        with pytest.raises(ValueError, match=msg):
            metrics.diff_map(a, a, **kw)
    small = np.zeros((10, 40, 3), np.uint8)
    with pytest.raises(ValueError, match=r"mode ssim needs frames of at least 11 x 11 \(got 10 x 40\)"):
        metrics.diff_map(small, small, mode="ssim")
    with pytest.raises(ValueError, match="at least 11 x 11"):
        metrics.ssim_map(small, small)
    with pytest.raises(AssertionError, match="the device was asked for"):
        metrics.diff_map(a, a)
    with pytest.raises(AssertionError, match="the device was asked for"):
        metrics.diff_map(small, small, mode="abs", gain=255, threshold=254, layout="side")  # no size limit outside the SSIM mode

    class Buf:
        ptr, nbytes = 0, 12 * 14 * 3

    with pytest.raises(ValueError, match="side frames and records need"):
        metrics.diff_map_launch(None, Buf(), Buf(), 1, 12, 14, Buf(), Buf(), layout="side")  # the output holds one panel, not three
    with pytest.raises(ValueError, match="d_ssim_map goes with mode ssim"):
        metrics.diff_map_launch(None, Buf(), Buf(), 1, 12, 14, Buf(), Buf(), mode="heat", d_ssim_map=Buf())
    with pytest.raises(ValueError):
        metrics.diff_map_launch(None, Buf(), Buf(), 17, 12, 14, Buf(), Buf())
    assert metrics.DiffRecord(7, 1, 2, 9) == metrics.DiffRecord(7, 1, 2, 9) != metrics.DiffRecord(7, 1, 2, 8)


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib, metrics

    fn = _lib.lib.avx_diff_map_u8
    assert "avx_diff_map_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 14 and fn.argtypes[7] is ctypes.c_float
    assert fn(None, None, None, 1, 16, 16, 1, 32.0, 1, 0, None, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context is refused first
    assert ctypes.sizeof(_lib.DiffRecord) == 16 == metrics.DIFF_RECORD_BYTES
    assert [f[0] for f in _lib.DiffRecord._fields_] == ["max_d", "max_x", "max_y", "beyond"]
    assert _lib.AVX_DIFF_MODES == {"abs": 0, "heat": 1, "ssim": 2} and _lib.AVX_DIFF_LAYOUTS == {"map": 0, "side": 1}
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert ("int avx_diff_map_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, int threshold,\n"
            "                    int layout, uint8_t* out_hwc, avx_diff_rec* rec_dev, float* ssim_map_dev, void* stream);") in hdr
    assert "enum avx_diff_mode { AVX_DIFF_ABS = 0, AVX_DIFF_HEAT = 1, AVX_DIFF_SSIM = 2 };" in hdr
    assert "enum avx_diff_layout { AVX_DIFF_MAP = 0, AVX_DIFF_SIDE = 1 };" in hdr
    assert "typedef struct { uint32_t max_d, max_x, max_y, beyond; } avx_diff_rec;" in hdr
    assert "#define AVX_ABI_VERSION 1" in hdr
    assert "diff_map.hip" in open(os.path.join(ROOT, "animal-vision_amd", "csrc", "Makefile")).read()
    # one copy of the float32 arithmetic of a position: both kernels call ssim_window.h's
    csrc = os.path.join(ROOT, "animal-vision_amd", "csrc")
    assert "ssim_position_f32" in open(os.path.join(csrc, "ssim_window.h")).read()
    for name in ("metrics.hip", "diff_map.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert "ssim_position_f32<" in src and "58.5225f" not in src, name
