"""CPU: dE_ITP (ITU-R BT.2124) -- the float64 definition of tests/_itp_ref.py against closed forms, the float32
restatement of csrc/itp.hip's arithmetic against the definition, the command's parser and its classification of inputs, and the
entry's declaration and binding.

The restatement on the frames of _itp_ref.CASES (the frames of tests/test_itp_gpu.py) is within 1.19e-3 of the definition (frame
pair "near" of p010le HLG limited against p010le PQ full at 70 x 530, where values reach 707: 1.7e-6 of the value); the GPU test
allows the device eight times the figure it measures, 9.5e-3.  For comparison: with the PQ EOTF in the form of the 8-bit decode
(c2 - c3 p, which cancels near the top) and the plain exp2(m2 log2 q) for the inverse, the same frames give 1.4e-2."""
import ctypes
import os
import re

import numpy as np
import pytest

import _itp_ref as I
import _rawyuv_ref as R
from animal_vision_amd import deltae as _deltae_module  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _neutral(Y, fmt="yuv444p10le"):
    """1 x n payload of neutral-chroma pixels with the given luma codes."""
    Y = np.asarray(Y).reshape(1, 1, -1)
    ch, cw = R.plane_shapes(fmt, 1, Y.shape[2])
    c = np.full((1, ch, cw), 512)
    return R.join_planes(Y, c, c, fmt)


# ------------------------------------------------------------------------------------------------ the definition
def test_grey_pq_pixels_one_luma_code_apart_are_720_over_876():
    codes = np.array([65, 100, 400, 512, 700, 939])  # above black: the PQ inverse of 0 nits is c1^m2 = 7.3e-7, not 0
    a, b = I.hdr(_neutral(codes), "yuv444p10le", "pq"), I.hdr(_neutral(codes + 1), "yuv444p10le", "pq")
    got = I.delta(a, b, 1, len(codes))
    assert np.abs(got - 720.0 / 876.0).max() <= 1e-9, got


def test_limited_range_peak_white_is_i_1_t_0_p_0():
    out = I.itp(I.nits_2020(I.hdr(_neutral([940]), "yuv444p10le", "pq"), 1, 1))[0, 0, 0]
    assert abs(out[0] - 1.0) <= 1e-12 and abs(out[1]) <= 1e-12 and abs(out[2]) <= 1e-12, out


def test_srgb_white_at_203_nits():
    out = I.itp(I.nits_2020(I.sdr(np.full((1, 1, 1, 3), 255, np.uint8)), 1, 1, 203.0))[0, 0, 0]
    assert abs(out[0] - I.pq_inverse(0.0203)) <= 1e-12 and abs(out[0] - 0.580689) <= 5e-7
    assert abs(out[1]) <= 1e-12 and abs(out[2]) <= 1e-12, out


def test_one_8bit_code_step_on_greys():
    for code, want in ((128, 1.14), (10, 3.22), (1, 12.56)):
        a, b = (I.sdr(np.full((1, 1, 1, 3), c, np.uint8)) for c in (code, code + 1))
        assert abs(I.delta(a, b, 1, 1)[0, 0, 0] - want) <= 5e-3, code


@pytest.mark.parametrize("case", I.CASES[2:7], ids=I.case_id)
def test_the_measure_is_symmetric(case):
    H, W = case[:2]
    sa, sb, want, f32v = I.case_sides(case)
    assert np.array_equal(I.delta(sb, sa, H, W), want)
    assert I.delta32(sb, sa, H, W).tobytes() == f32v.tobytes()


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic
def test_restatement_against_the_definition_on_the_test_frames():
    worst = 0.0
    for case in I.CASES:
        sa, sb, want, f32v = I.case_sides(case)
        dev = np.abs(f32v.astype(np.float64) - want).reshape(len(I.KINDS), -1).max(1)
        print(f"itp restatement {I.case_id(case)}: " + ", ".join(f"{k} {d:.3e}" for k, d in zip(I.KINDS, dev)) + f"; largest dE_ITP {want.max():.2f}")
        worst = max(worst, float(dev.max()))
    print(f"itp restatement: largest deviation {worst:.3e}; the GPU bound is 8 x that, {8 * worst:.3e}")
    assert worst == I.restatement_deviation()
    assert worst <= 2e-3  # float32 in this form: about 2e-6 of values that reach 700; the plain forms give 1.4e-2


def test_restatement_keeps_the_exact_cases():
    g = np.arange(256, dtype=np.uint8)
    grey = np.repeat(g[None, None, :, None], 3, axis=3)  # 1 x 1 x 256 x 3
    i, t, p = I.itp32(I.sdr(grey), 1, 256)
    assert not t.any() and not p.any() and (np.diff(i[0, 0]) > 0).all()
    for tr, rng in (("pq", "limited"), ("hlg", "full")):
        i, t, p = I.itp32(I.hdr(_neutral(np.arange(1024)), "yuv444p10le", tr, rng), 1, 1024)
        assert not t.any() and not p.any(), (tr, rng)
    d = I.delta32(I.sdr(grey), I.sdr(grey[:, :, ::-1]), 1, 256)
    assert d.tobytes() == np.abs(I.itp32(I.sdr(grey), 1, 256)[0] - I.itp32(I.sdr(grey[:, :, ::-1]), 1, 256)[0]).tobytes()
    assert not I.delta32(I.sdr(grey), I.sdr(grey), 1, 256).any()


# ------------------------------------------------------------------------------------------------ the parser
def _error(capsys, argv):
    from animal_vision_amd import deltae

    with pytest.raises(SystemExit) as e:
        deltae.parse_args(argv)
    assert e.value.code == 2, argv
    return capsys.readouterr().err


def test_parser_refusals_by_name(capsys):
    hdr = ["a.yuv", "b.y4m", "--pix-fmt", "p010le", "--size", "16x16", "--transfer", "pq", "--itp"]
    assert "--itp and --ppd do not combine" in _error(capsys, hdr + ["--ppd", "60"])
    assert "--itp and --observer do not combine" in _error(capsys, hdr + ["--observer", "Dog", "--weber", "0.05,0.05"])
    assert "--itp and --acuity do not combine" in _error(capsys, hdr + ["--acuity", "2"])
    assert "--itp and --scale do not combine" in _error(capsys, hdr + ["--scale", "8x8"])
    err = _error(capsys, ["a.yuv", "b.y4m", "--pix-fmt", "p010le", "--size", "16x16", "--itp"])
    assert "--itp: a.yuv is raw p010le video, an HDR side" in err and "--transfer" in err
    err = _error(capsys, ["a.y4m", "b.yuv", "--pix-fmt", "yuv420p10le", "--size", "16x16", "--itp"])
    assert "--itp: b.yuv is raw yuv420p10le video, an HDR side" in err
    assert "--sdr-white must be finite and positive" in _error(capsys, ["a.npy", "b.npy", "--itp", "--sdr-white", "-1"])
    assert "--sdr-white needs --transfer" in _error(capsys, ["a.npy", "b.npy", "--sdr-white", "100"])  # without --itp: as it was


def test_inputs_are_classified_as_hdr_or_sdr(tmp_path):
    from animal_vision_amd import deltae

    frames = tmp_path / "frames"
    frames.mkdir()
    a = deltae.parse_args(["a.yuv", "b.y4m", "--pix-fmt", "p010le", "--size", "16x16", "--transfer", "pq", "--itp"])
    assert a.itp and a.itp_kinds == ("hdr", "sdr") and a.sdr_white == 203.0
    for path, kind in (("a.yuv", "hdr"), ("clip.raw", "hdr"), ("-", "hdr"), ("b.y4m", "sdr"), ("B.Y4M", "sdr"), ("c.npy", "sdr"), ("synthetic:16x16:2", "sdr"),
                       (str(frames), "sdr")):
        assert deltae.itp_side_kind(a, path) == kind, path
    a = deltae.parse_args(["a.yuv", "b.yuv", "--pix-fmt", "nv12", "--size", "16x16", "--itp", "--sdr-white", "100"])  # 8-bit raw video: SDR
    assert a.itp_kinds == ("sdr", "sdr") and a.sdr_white == 100.0 and a.transfer is None
    a = deltae.parse_args(["a.npy", "b.y4m", "--itp"])
    assert a.itp_kinds == ("sdr", "sdr") and a.sdr_white == 203.0
    a = deltae.parse_args(["a.yuv", "b.yuv", "o.y4m", "--pix-fmt", "yuv444p10le", "--size", "16x16", "--transfer", "hlg", "--itp", "--tonemap", "clip",
                           "--sdr-white", "100"])
    assert a.itp_kinds == ("hdr", "hdr") and (a.transfer, a.tonemap, a.sdr_white) == ("hlg", "clip", 100.0)
    a = deltae.parse_args(["a.yuv", "b.y4m", "--pix-fmt", "p010le", "--size", "16x16", "--transfer", "pq"])
    assert not a.itp and not hasattr(a, "itp_kinds")


def test_hdr_frames_and_options_are_checked_before_the_device():
    from animal_vision_amd import metrics

    fsz = R.frame_size("p010le", 4, 6)
    h = metrics.HdrFrames(np.zeros((3, fsz), np.uint8), "p010le", 4, 6, "pq")
    assert len(h) == 3 and h.batched and (h.pix_fmt, h.H, h.W, h.transfer, h.range) == ("p010le", 4, 6, "pq", "limited")
    one = metrics.HdrFrames(np.zeros(fsz // 2, "<u2"), "p010le", 4, 6, "hlg", "full")
    assert len(one) == 1 and not one.batched and one.payload.dtype == np.uint8 and one.payload.shape == (1, fsz)
    for bad in (dict(pix_fmt="nv12"), dict(pix_fmt="yuv420p"), dict(transfer="gamma"), dict(range="tv")):
        kw = dict(pix_fmt="p010le", transfer="pq", range="limited")
        kw.update(bad)
        with pytest.raises(ValueError):
            metrics.HdrFrames(np.zeros(fsz, np.uint8), kw["pix_fmt"], 4, 6, kw["transfer"], kw["range"])
    with pytest.raises(ValueError, match="bytes per 4x6 p010le frame"):
        metrics.HdrFrames(np.zeros(fsz + 2, np.uint8), "p010le", 4, 6, "pq")
    for white in (0.0, -203.0, float("nan"), float("inf"), "203", True):
        with pytest.raises(ValueError, match="sdr_white"):
            metrics.check_sdr_white(white)
    assert metrics.check_sdr_white(100) == 100.0 and metrics.ITP_DEFAULT_SDR_WHITE == 203.0


# ------------------------------------------------------------------------------------------------ the library
def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib, metrics

    fn = _lib.lib.avx_itp_delta
    assert "avx_itp_delta" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    side = _lib.ItpSide(struct_size=ctypes.sizeof(_lib.ItpSide))
    assert fn(None, ctypes.byref(side), ctypes.byref(side), 203.0, 1, 16, 16, 0, 10.0, 1.0, 0, None, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context
    assert ctypes.sizeof(_lib.ItpSide) == 40 and [f[0] for f in _lib.ItpSide._fields_] == ["struct_size", "kind", "data", "panel", "pix_fmt", "full_range",
                                                                                           "transfer", "reserved"]
    assert (_lib.ItpSide.data.offset, _lib.ItpSide.panel.offset, _lib.ItpSide.pix_fmt.offset, _lib.ItpSide.transfer.offset) == (8, 16, 24, 32)
    assert _lib.AVX_ITP_KINDS == {"sdr": 0, "hdr": 1}
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert re.search(r"int avx_itp_delta\(avx_ctx\* ctx, const avx_itp_side\* a, const avx_itp_side\* b, double sdr_white, int n_frames, int H, int W,", hdr)
    assert "enum avx_itp_kind { AVX_ITP_SDR = 0, AVX_ITP_HDR = 1 };" in hdr and "typedef struct avx_itp_side {" in hdr
    mk = open(os.path.join(ROOT, "animal-vision_amd", "csrc", "Makefile")).read()
    assert " itp.hip " in mk
    for name in ("HdrFrames", "ItpSide", "itp_delta", "itp_delta_map", "itp_delta_values", "itp_delta_launch"):
        assert hasattr(metrics, name), name
