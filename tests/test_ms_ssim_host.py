"""No GPU: the host side of MS-SSIM -- the float64 yardstick of tests/_ms_ssim_ref.py against itself, the arithmetic of
metrics.MsSsim on hand-written records, the record's size, and the parser of compare --ms-ssim (the device loop stubbed)."""
import ctypes
import math
import os

import numpy as np
import pytest

import _metrics_ref as R
import _ms_ssim_ref as M
from animal_vision_amd import compare, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the yardstick
def test_reference_identical_frames_give_exactly_one():
    a = R.six_frames(177, 207, seed=3)[0][1]
    cs, ss = M.levels(a, a)
    assert (cs == 1.0).all() and (ss == 1.0).all()
    assert M.ms_ssim_channels(a, a) == [1.0, 1.0, 1.0] and M.ms_ssim(a, a) == 1.0


def test_reference_flat255_against_flat254_closed_form():
    _, a, b = R.six_frames(176, 176)[2]
    cs, ss = M.levels(a, b)
    assert (cs == 1.0).all()  # both variances and the covariance are 0 at every scale
    l = (2.0 * 255.0 * 254.0 + R.C1) / (255.0 ** 2 + 254.0 ** 2 + R.C1)  # 129546.5025 / 129547.5025
    assert np.abs(ss - l).max() < 1e-12
    for v in M.ms_ssim_channels(a, b):
        assert abs(v - l ** 0.1333) < 1e-12
    assert abs(M.ms_ssim(a, b) - 0.999998971) < 1e-9


def test_reference_block_sums_equal_successive_pooling():
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, (177, 207), dtype=np.uint8)
    pyr = M.pyramid(x)
    assert [p.shape for p in pyr] == [(177, 207), (88, 103), (44, 51), (22, 25), (11, 12)]
    for j, p in enumerate(pyr):
        s = M.block_sums(x, j)
        assert s.max() <= 255 * 4 ** j <= 65280
        assert (s.astype(np.float64) / 4.0 ** j).tobytes() == p.tobytes(), j


def test_reference_values_of_the_known_pairs_and_minimum_size():
    pairs = {n: (a, b) for n, a, b in R.six_frames(176, 176)}
    cs, ss = M.levels(*pairs["inverse"])
    assert cs[0, 0] < -0.98 and M.ms_ssim(*pairs["inverse"]) == 0.0  # a negative mean is clamped in the product alone
    cs, ss = M.levels(*pairs["ramp_noise8"])
    assert cs[0, 0] < 0.76 and cs[0, 2] > 0.99  # what single-scale SSIM sees of pixel noise, and what scale 2 sees
    assert abs(M.combine(cs[0], ss[0]) - 0.968539124) < 1e-8
    assert M.MIN_SIDE == 176
    for shape in ((175, 176), (176, 175)):
        with pytest.raises(ValueError, match="176"):
            M.pyramid(np.zeros(shape, np.uint8))


# ------------------------------------------------------------------------------------------------ MsSsim
def test_ms_ssim_arithmetic_on_hand_written_records():
    assert metrics.MS_WEIGHTS == M.WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) and abs(sum(metrics.MS_WEIGHTS) - 1.0001) < 1e-12
    cs = np.array([[0.5, 0.6, 0.7, 0.8, 0.9], [1.0] * 5, [0.9, -0.25, 0.8, 0.7, 0.6]])
    ss = np.array([[0.4, 0.5, 0.6, 0.7, 0.81], [1.0] * 5, [0.8, -0.3, 0.7, 0.6, 0.5]])
    m = metrics.MsSsim(cs, ss)
    want0 = 0.5 ** 0.0448 * 0.6 ** 0.2856 * 0.7 ** 0.3001 * 0.8 ** 0.2363 * 0.81 ** 0.1333
    ch = m.ms_ssim_channels
    assert ch[0] == pytest.approx(want0, rel=1e-14) and ch[1] == 1.0 and ch[2] == 0.0  # a negative cs makes the product 0.0
    assert m.ms_ssim == pytest.approx((want0 + 1.0) / 3.0, rel=1e-14)
    assert m.cs[2][1] == -0.25  # the stored means are not clamped
    neg4 = metrics.MsSsim(np.ones((3, 5)), np.array([[1, 1, 1, 1, -0.1]] * 3))
    assert neg4.ms_ssim_channels == (0.0, 0.0, 0.0) and neg4.ms_ssim == 0.0
    assert metrics.MsSsim(np.full((3, 5), -1.0), ss).ms_ssim == 0.0
    for c in range(3):
        assert ch[c] == pytest.approx(M.combine(cs[c], ss[c]), rel=1e-14)
    # equality is on bytes: -0.0 is not 0.0, NaN equals the same NaN
    assert m == metrics.MsSsim(cs.copy(), ss.copy()) and m != metrics.MsSsim(cs + np.eye(3, 5) * 1e-9, ss)
    z, nz = np.zeros((3, 5)), np.zeros((3, 5))
    nz[0, 0] = -0.0
    assert metrics.MsSsim(z, z) != metrics.MsSsim(nz, z)
    nan = np.full((3, 5), math.nan)
    assert metrics.MsSsim(nan, nan) == metrics.MsSsim(nan.copy(), nan.copy())
    assert (m == 3) is False
    with pytest.raises(ValueError, match="3 x 5"):
        metrics.MsSsim(np.zeros((3, 4)), ss)
    assert "ms_ssim=" in repr(m)


def test_record_layout_and_symbol():
    from animal_vision_amd import _lib

    assert ctypes.sizeof(_lib.MsSsimRecord) == 240 == metrics.MS_RECORD_BYTES
    assert _lib.MsSsimRecord.cs.offset == 0 and _lib.MsSsimRecord.ssim.offset == 120
    fn = _lib.lib.avx_frame_metrics_ms_u8
    assert "avx_frame_metrics_ms_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn(None, None, None, 1, 176, 176, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context is refused first
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert "typedef struct avx_ms_ssim_rec {" in hdr and "double cs[3][5];" in hdr and "double ssim[3][5];" in hdr
    assert ("int avx_frame_metrics_ms_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W,\n"
            "                            avx_frame_metrics* out_dev, avx_ms_ssim_rec* ms_out_dev, void* stream);") in hdr
    assert "ms_ssim.hip" in open(os.path.join(ROOT, "animal-vision_amd", "csrc", "Makefile")).read()
    # records_from_bytes' counterpart reads [channel][scale] doubles, cs first
    raw = np.arange(60, dtype=np.float64)
    recs = metrics.ms_records_from_bytes(raw.view(np.uint8), 2)
    assert len(recs) == 2 and recs[0].cs[1][2] == 7.0 and recs[0].ssim[0][0] == 15.0 and recs[1].cs[0][0] == 30.0 and recs[1].ssim[2][4] == 59.0


def test_small_frames_are_refused_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    for shape in ((175, 176, 3), (176, 175, 3), (2, 100, 300, 3)):
        with pytest.raises(ValueError, match="176"):
            metrics.ms_ssim(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8))
    with pytest.raises(ValueError, match=r"\(176, 176, 3\).*\(176, 177, 3\)"):
        metrics.ms_ssim(np.zeros((176, 176, 3), np.uint8), np.zeros((176, 177, 3), np.uint8))
    with pytest.raises(AssertionError, match="the device was asked for"):
        metrics.ms_ssim(np.zeros((176, 176, 3), np.uint8), np.zeros((176, 176, 3), np.uint8))

    class Buf:
        ptr, nbytes = 0, 1 << 30

    for n, H, W in ((1, 175, 176), (1, 176, 175), (0, 176, 176), (17, 176, 176)):
        with pytest.raises(ValueError):
            metrics.frame_metrics_ms_device(None, Buf(), Buf(), n, H, W)
        with pytest.raises(ValueError):
            metrics.frame_metrics_ms_launch(None, Buf(), Buf(), n, H, W, Buf(), Buf())


# ------------------------------------------------------------------------------------------------ the parser and the command
def test_parser_flag_header_and_refusals(capsys):
    a = compare.parse_args(["a.npy", "b.npy"])
    assert not hasattr(a, "ms_ssim") and not hasattr(a, "min_ms_ssim")  # without the flag the namespace is what it was
    a = compare.parse_args(["a.npy", "b.npy", "--ms-ssim"])
    assert a.ms_ssim is True and not hasattr(a, "min_ms_ssim")
    a = compare.parse_args(["a.npy", "b.npy", "--min-ms-ssim", "0.95"])
    assert a.ms_ssim is True and a.min_ms_ssim == 0.95
    a = compare.parse_args(["a.yuv", "b.yuv", "--pix-fmt", "nv12", "--size", "3840x2160", "--scale", "176x176", "--ms-ssim"])
    assert a.ms_ssim is True and a.scale == (176, 176)
    assert compare.CSV_HEADER + compare.CSV_MS_COLUMNS == ("frame,psnr_r,psnr_g,psnr_b,psnr,ssim_r,ssim_g,ssim_b,ssim,max_abs,beyond1,"
                                                            "ms_ssim_r,ms_ssim_g,ms_ssim_b,ms_ssim")
    for bad, words in ((["a.npy", "b.npy", "--ms-ssim", "--no-ssim"], ("--ms-ssim", "--no-ssim")),
                       (["a.npy", "b.npy", "--min-ms-ssim", "0.9", "--no-ssim"], ("--ms-ssim", "--no-ssim")),
                       (["a.y4m", "b.y4m", "--ms-ssim", "--planes", "yuv"], ("--ms-ssim", "--planes yuv")),
                       (["a.yuv", "b.yuv", "--pix-fmt", "nv12", "--size", "640x480", "--scale", "320x175", "--ms-ssim"], ("--ms-ssim", "176x176", "320x175")),
                       (["a.yuv", "b.yuv", "--pix-fmt", "nv12", "--size", "174x480", "--ms-ssim"], ("--ms-ssim", "176x176", "174x480")),
                       (["synthetic:160x120:2", "synthetic:160x120:2", "--ms-ssim"], ("--ms-ssim", "176x176", "160x120"))):
        with pytest.raises(SystemExit) as e:
            compare.parse_args(bad)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (bad, err)


def _frame_record(ssim=(1.0, 1.0, 1.0), diffs=None):
    h = np.zeros((3, 256), np.uint64)
    h[:, 0] = 100
    for k, cnt in (diffs or {}).items():
        h[:, k], h[:, 0] = cnt, 100 - cnt
    return metrics.FrameMetrics(h, ssim)


def _run(monkeypatch, capsys, items, argv):
    seen = {}

    def stub(args, info):
        seen["ms"] = getattr(args, "ms_ssim", False)
        yield from items

    monkeypatch.setattr(compare, "stream_metrics", stub)
    status = compare.main(["a.npy", "b.npy"] + argv)
    cap = capsys.readouterr()
    return status, cap.out.splitlines(), cap.err, seen["ms"]


def test_command_columns_summary_and_limit(monkeypatch, capsys):
    one = metrics.MsSsim(np.ones((3, 5)), np.ones((3, 5)))
    low = metrics.MsSsim(np.full((3, 5), 0.5), np.full((3, 5), 0.5))
    v = low.ms_ssim
    assert v == pytest.approx(0.5 ** sum(metrics.MS_WEIGHTS))
    recs = [_frame_record(), _frame_record((0.9, 0.9, 0.9), {1: 10})]
    status, plain, err_plain, ms = _run(monkeypatch, capsys, recs, [])
    assert status == 0 and ms is False and plain[0] == compare.CSV_HEADER and "MS-SSIM" not in err_plain
    status, out, err, ms = _run(monkeypatch, capsys, list(zip(recs, [one, low])), ["--ms-ssim"])
    assert status == 0 and ms is True and out[0] == compare.CSV_HEADER + compare.CSV_MS_COLUMNS
    assert [line.rsplit(",", 4)[0] for line in out] == plain  # the other columns are what the run without the flag prints
    assert out[1].split(",")[-4:] == ["1.000000"] * 4 and out[2].split(",")[-4:] == [f"{v:.6f}"] * 4
    assert f"MS-SSIM mean {(1.0 + v) / 2:.6f} min {v:.6f}" in err and "SSIM mean 0.950000 min 0.900000" in err
    status, out, err, ms = _run(monkeypatch, capsys, list(zip(recs, [one, low])), ["--min-ms-ssim", "0.9"])
    assert status == 1 and ms is True and len(out) == 3 and "compare: frame 1: MS-SSIM" in err and "--min-ms-ssim 0.9" in err
    status, out, err, ms = _run(monkeypatch, capsys, list(zip(recs, [one, low])), ["--min-ms-ssim", "0.2"])
    assert status == 0 and "compare: frame" not in err
    status, out, err, ms = _run(monkeypatch, capsys, list(zip(recs, [one, one])), ["--ms-ssim", "--min-ssim", "0.95"])
    assert status == 1 and "compare: frame 1: SSIM" in err  # the other limits still act
