"""No GPU: the host side of the frame metrics and the compare command -- the float64 yardstick agrees with itself, the
derived figures of FrameMetrics on hand-made histograms, the command's parser and exit-status rules (the device loop stubbed), and the
exported symbol with its prototype."""
import ctypes
import math
import os

import numpy as np
import pytest

import _metrics_ref as R
from animal_vision_amd import compare as _compare_module, metrics as _metrics_module  # noqa: F401  (the feature: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the yardstick
def test_reference_sse_from_histogram_is_the_sum_of_squares():
    for name, a, b in R.six_frames(23, 31):
        h = R.abs_hist(a, b)
        assert [int(v) for v in h.sum(axis=1)] == [23 * 31] * 3, name
        d = a.astype(np.int64) - b.astype(np.int64)
        assert R.sse_from_hist(h) == [int((d[..., c] ** 2).sum()) for c in range(3)], name


def test_reference_identical_frames():
    a = R.six_frames(19, 27)[0][1]
    assert R.sse_from_hist(R.abs_hist(a, a)) == [0, 0, 0]
    assert R.psnr(0, a.size) == math.inf
    assert R.ssim(a, a) == [1.0, 1.0, 1.0]


def test_reference_black_against_white_closed_form():
    a, b = np.zeros((16, 20, 3), np.uint8), np.full((16, 20, 3), 255, np.uint8)
    want = R.C1 / (255.0 ** 2 + R.C1)  # mu_a = 0, every variance 0: (C1 * C2) / ((255^2 + C1) * C2)
    for v in R.ssim(a, b):
        assert abs(v - want) < 1e-12
    assert R.psnr(R.sse_from_hist(R.abs_hist(a, b))[0], 16 * 20) == 0.0


def test_reference_small_frames_have_no_ssim():
    a = np.zeros((10, 40, 3), np.uint8)
    assert all(math.isnan(v) for v in R.ssim(a, a))
    assert abs(R.taps().sum() - 1.0) < 1e-15 and len(R.taps()) == 11


# ------------------------------------------------------------------------------------------------ FrameMetrics
def test_frame_metrics_properties_on_hand_made_histograms():
    from animal_vision_amd.metrics import FrameMetrics

    h = np.zeros((3, 256), np.uint64)
    h[0, 0], h[0, 1], h[0, 3] = 90, 8, 2          # SSE 8 + 18 = 26
    h[1, 0] = 100                                  # identical channel
    h[2, 0], h[2, 255] = 99, 1                     # SSE 65025
    m = FrameMetrics(h, (0.5, 1.0, 0.75))
    assert m.samples == 100
    assert m.sse == (26, 0, 65025)
    p = m.psnr_channels
    assert p[0] == pytest.approx(10 * math.log10(255.0 ** 2 * 100 / 26)) and p[1] == math.inf and p[2] == pytest.approx(20.0)
    assert m.psnr == pytest.approx(10 * math.log10(255.0 ** 2 * 300 / (26 + 65025)))
    assert m.max_abs == 255
    assert m.count_beyond(1) == 3 and m.share_beyond(1) == 3 / 300 and m.share_beyond(0) == 11 / 300 and m.share_beyond(255) == 0.0
    assert m.ssim_mean == 0.75
    same = FrameMetrics(np.pad(np.full((3, 1), 7, np.uint64), ((0, 0), (0, 255))))
    assert same.psnr == math.inf and same.max_abs == 0 and same.share_beyond(0) == 0.0 and all(math.isnan(v) for v in same.ssim)
    with pytest.raises(ValueError):
        FrameMetrics(np.zeros((3, 255)))
    # counts beyond uint32 stay exact (k^2 * count above 2^53 would not in float64)
    big = np.zeros((3, 256), np.uint64)
    big[0, 255] = (1 << 32) - 1
    assert FrameMetrics(big).sse[0] == 255 * 255 * ((1 << 32) - 1)


def test_frame_metrics_refuses_mismatched_inputs_before_the_device(monkeypatch):
    from animal_vision_amd import metrics

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    a = np.zeros((12, 14, 3), np.uint8)
    with pytest.raises(ValueError, match=r"\(12, 14, 3\).*\(12, 15, 3\)"):
        metrics.frame_metrics(a, np.zeros((12, 15, 3), np.uint8))
    with pytest.raises(ValueError, match=r"uint8.*float32"):
        metrics.frame_metrics(a, a.astype(np.float32))
    with pytest.raises(ValueError, match=r"\(2, 12, 14, 3\)"):
        metrics.frame_metrics(a, np.zeros((2, 12, 14, 3), np.uint8))
    with pytest.raises(ValueError):
        metrics.frame_metrics(a[..., :2], a[..., :2])
    with pytest.raises(AssertionError, match="the device was asked for"):
        metrics.frame_metrics(a, a)

    class Buf:
        ptr, nbytes = 0, 100

    for n, H, W in ((0, 4, 4), (17, 4, 4), (1, 0, 4), (1, 4, 4 + 100)):  # n_frames, a bad size, undersized buffers
        with pytest.raises(ValueError):
            metrics.frame_metrics_device(None, Buf(), Buf(), n, H, W)


# ------------------------------------------------------------------------------------------------ the parser
def test_parser_shared_options_and_limits():
    from animal_vision_amd import compare

    a = compare.parse_args(["a.y4m", "b.npy"])
    assert (a.a, a.b, a.batch, a.no_ssim, a.shortest, a.csv, a.matrix, a.scale) == ("a.y4m", "b.npy", 8, False, False, None, "bt601", None)
    a = compare.parse_args(["a.yuv", "b.yuv", "--pix-fmt", "nv12", "--size", "64x48", "--matrix", "bt709", "--range", "full", "--scale", "32x24",
                            "--batch", "16", "--no-ssim", "--max-abs", "1", "--max-beyond1", "0.002", "--min-psnr", "40"])
    assert (a.pix_fmt, a.size, a.matrix, a.range, a.scale, a.batch, a.no_ssim) == ("nv12", (64, 48), "bt709", "full", (32, 24), 16, True)
    assert (a.max_abs, a.max_beyond1, a.min_psnr, a.min_ssim) == (1, 0.002, 40.0, None)
    a = compare.parse_args(["a.yuv", "b.yuv", "--pix-fmt", "p010le", "--size", "64x48", "--transfer", "pq", "--tonemap", "clip", "--peak-nits", "600"])
    assert (a.transfer, a.tonemap, a.peak_nits, a.sdr_white) == ("pq", "clip", 600.0, 203.0)
    for bad in (["a.y4m", "b.y4m", "--batch", "0"], ["a.y4m", "b.y4m", "--batch", "17"],
                ["a.y4m", "b.y4m", "--out-pix-fmt", "nv12"], ["a.y4m", "b.y4m", "--out-matrix", "bt709"], ["a.y4m", "b.y4m", "--depth", "2"],
                ["a.y4m", "b.y4m", "--species", "Dog"], ["a.y4m"], ["a.y4m", "b.y4m", "--pix-fmt", "nv12"], ["a.y4m", "b.y4m", "--tonemap", "clip"],
                ["a.y4m", "b.y4m", "--no-ssim", "--min-ssim", "0.9"], ["-", "-"],
                ["synthetic:64x48:2", "synthetic:32x24:2", "--scale", "64x48"], ["synthetic:32x24:2", "synthetic:64x48:2", "--scale", "64x48"]):
        with pytest.raises(SystemExit) as e:
            compare.parse_args(bad)
        assert e.value.code == 2, bad


# ------------------------------------------------------------------------------------------------ exit status
def _record(diffs, ssim=(1.0, 1.0, 1.0), n=100):
    from animal_vision_amd.metrics import FrameMetrics

    h = np.zeros((3, 256), np.uint64)
    for c in range(3):
        for k, cnt in diffs.items():
            h[c, k] = cnt
        h[c, 0] = n - sum(diffs.values())
    return FrameMetrics(h, ssim)


def _run(monkeypatch, capsys, records, argv, longer=None):
    from animal_vision_amd import compare

    def stub(args, info):
        if longer:
            info["longer"] = longer
        yield from records

    monkeypatch.setattr(compare, "stream_metrics", stub)
    status = compare.main(["a.npy", "b.npy"] + argv)
    cap = capsys.readouterr()
    return status, cap.out.splitlines(), cap.err


def test_exit_status_rules(monkeypatch, capsys, tmp_path):
    from animal_vision_amd import compare

    same, off1, off3 = _record({}), _record({1: 10}, (0.99, 0.99, 0.99)), _record({1: 1, 3: 1}, (0.9, 0.95, 1.0))
    status, out, err = _run(monkeypatch, capsys, [same, same], [])
    assert status == 0 and out[0] == compare.CSV_HEADER and len(out) == 3
    assert out[1] == "0,inf,inf,inf,inf,1.000000,1.000000,1.000000,1.000000,0,0" and out[2].startswith("1,inf,")
    assert "compare: 2 frames, PSNR inf dB" in err and "largest difference 0" in err and "fps" in err
    # no limit given: differences are reported, not judged
    status, out, err = _run(monkeypatch, capsys, [same, off3], [])
    assert status == 0 and out[2].split(",")[9:] == ["3", "0.01"]
    want = 10 * math.log10(255.0 ** 2 * 600 / (3 * 10))  # pooled over both frames: SSE 3 * (1 + 9) in 600 samples
    assert f"PSNR {want:.6f} dB" in err and "SSIM mean 0.975000 min 0.950000" in err and "largest difference 3" in err
    for argv, bad_frame in ((["--max-abs", "2"], 2), (["--max-abs", "0"], 1), (["--max-beyond1", "0.005"], 2), (["--min-ssim", "0.96"], 2),
                            (["--min-psnr", "60"], 1), (["--min-psnr", "50"], None), (["--max-abs", "3", "--max-beyond1", "0.01"], None)):
        status, out, err = _run(monkeypatch, capsys, [same, off1, off3], argv)
        assert len(out) == 4, argv  # every frame is still reported
        if bad_frame is None:
            assert status == 0 and "compare: frame" not in err, (argv, err)
        else:
            assert status == 1 and f"compare: frame {bad_frame}:" in err, (argv, err)
    # different lengths: status 2 and a remark, unless --shortest; a violated limit still wins
    status, out, err = _run(monkeypatch, capsys, [same], [], longer="B")
    assert status == 2 and "B has more frames" in err and "first 1" in err
    status, out, err = _run(monkeypatch, capsys, [same], ["--shortest"], longer="B")
    assert status == 0 and "more frames" not in err
    status, out, err = _run(monkeypatch, capsys, [off1], ["--max-abs", "0"], longer="A")
    assert status == 1 and "A has more frames" in err
    # --csv FILE takes the lines; --no-ssim reads nan and skips the SSIM summary
    path = tmp_path / "q.csv"
    nos = _record({2: 4}, (math.nan,) * 3)
    status, out, err = _run(monkeypatch, capsys, [nos], ["--csv", str(path), "--no-ssim"])
    assert status == 0 and out == [] and "SSIM skipped" in err
    lines = path.read_text().splitlines()
    assert lines[0] == compare.CSV_HEADER and lines[1].split(",")[5:9] == ["nan"] * 4 and lines[1].split(",")[9] == "2"


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib, metrics

    fn = _lib.lib.avx_frame_metrics_u8
    assert "avx_frame_metrics_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn(None, None, None, 1, 16, 16, 1, None, None) == _lib.AVX_ERR_INVALID  # a NULL context is refused first
    assert ctypes.sizeof(_lib.FrameMetricsRecord) == 3 * 256 * 4 + 3 * 8 == metrics.RECORD_BYTES
    assert _lib.FrameMetricsRecord.ssim.offset == 3072
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert ("int avx_frame_metrics_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W,\n"
            "                         int with_ssim, avx_frame_metrics* out_dev, void* stream);") in hdr
    assert "uint32_t abs_hist[3][256];" in hdr and "double   ssim[3];" in hdr and "} avx_frame_metrics;" in hdr
    assert "#define AVX_ABI_VERSION 1" in hdr
    assert "metrics.hip" in open(os.path.join(ROOT, "animal-vision_amd", "csrc", "Makefile")).read()
