"""CPU: the HDR decode of DESIGN §4.10 -- the float64 definition (tests/_hdr_ref.py) pinned to the standards and to exact anchors,
the error budget of the device's float32 arithmetic (restated here in NumPy, operation for operation as csrc/yuv_hdr.hip does
it) against the definition, the argument checks that need no device, the `video` command's option errors and the ABI symbols.
No device is used."""
import ctypes
import os
import re

import numpy as np
import pytest

import _hdr_ref as H
import _rawyuv_ref as R
from conftest import ROOT


# ---------------------------------------------------------------- the definition against the standards --------------------------
def test_pq_eotf_at_the_tabulated_points():
    # ST 2084 / BT.2100 table: E' = 0 -> 0, E' = 0.5081 -> ~100 cd/m2 (the 10-bit code 520 region), E' = 1 -> 10000
    assert H.pq_eotf(0.0) == 0.0
    assert H.pq_eotf(1.0) == pytest.approx(10000.0, rel=1e-12)
    assert H.pq_eotf(0.5081) == pytest.approx(100.0, rel=2e-3)
    # the inverse at 100 nits: N = ((c1 + c2 L^m1) / (1 + c3 L^m1))^m2 = 0.508078...
    L = (100.0 / 10000.0) ** H.PQ_M1
    n = ((H.PQ_C1 + H.PQ_C2 * L) / (1.0 + H.PQ_C3 * L)) ** H.PQ_M2
    assert n == pytest.approx(0.5081, abs=5e-5) and H.pq_eotf(n) == pytest.approx(100.0, rel=1e-10)
    assert H.PQ_C1 == pytest.approx(H.PQ_C3 - H.PQ_C2 + 1.0, abs=1e-15)  # the standard's own identity


def test_hlg_at_the_tabulated_points():
    assert H.hlg_inverse_oetf(0.5) == pytest.approx(1.0 / 12.0, rel=1e-15)
    assert H.hlg_inverse_oetf(1.0) == pytest.approx(1.0, abs=1e-7)   # a, b, c are given to 8 digits
    assert H.hlg_inverse_oetf(0.0) == 0.0
    e = 0.5 + 1e-9  # the two branches meet
    assert H.hlg_inverse_oetf(e) == pytest.approx(e * e / 3.0, rel=1e-7)
    grey = H.hlg_to_nits(np.array([1.0, 1.0, 1.0]))
    assert np.allclose(grey, 1000.0, rtol=1e-6) and grey[0] == grey[1] == grey[2]
    assert (H.hlg_to_nits(np.zeros(3)) == 0.0).all()
    assert H.LUM.sum() == pytest.approx(1.0, abs=1e-15)


def test_gamut_matrix_rows_sum_to_one_and_709_lies_inside_2020():
    M = H.gamut_matrix()
    assert np.abs(M.sum(1) - 1.0).max() <= 1e-15
    # BT.2087's published matrix, to its four digits
    want = np.array([[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]])
    assert np.abs(M - want).max() < 5e-5
    inv = np.linalg.inv(M)  # columns: the 709 primaries in 2020 coordinates -- inside the triangle: all weights in [0, 1]
    assert (inv >= 0.0).all() and (inv <= 1.0).all() and np.abs(inv.sum(1) - 1.0).max() < 1e-14
    # the difference form keeps a neutral pixel exactly neutral and equals the plain product elsewhere
    x = np.random.default_rng(0).random((1000, 3))
    assert np.allclose(H.gamut(x), np.clip(x @ M.T, 0, 1), atol=1e-14)
    n = np.repeat(np.random.default_rng(1).random((1000, 1)), 3, 1)
    assert np.array_equal(H.gamut(n), n)


@pytest.mark.parametrize("P", [1000.0 / 203.0, 4000.0 / 203.0, 1.5])
def test_mobius_curve(P):
    k = H.KNEE
    t = lambda m: H.tone_curve(m, "mobius", P)  # noqa: E731
    below = np.linspace(0.0, k, 1001)
    assert np.array_equal(t(below), below)
    h = 1e-7
    assert t(k + h) == pytest.approx(k + h, abs=1e-12)                         # continuous at the knee
    assert (t(k + h) - t(k)) / h == pytest.approx(1.0, abs=1e-5)                 # C1: the one-sided slopes agree
    assert (t(k) - t(k - h)) / h == pytest.approx(1.0, abs=1e-9)
    grid = np.linspace(0.0, 1.5 * P, 200001)
    v = t(grid)
    assert (np.diff(v) >= 0.0).all() and v.max() <= 1.0
    assert (np.diff(v[grid < P]) > 0.0).all()
    assert t(P) == pytest.approx(1.0, abs=1e-15) and t(10.0 * P) == t(P)
    c = H.tone_curve(grid, "clip", P)
    assert np.array_equal(c, np.minimum(grid, 1.0))


def test_tone_map_preserves_hue():
    v = np.random.default_rng(2).random((1000, 3)) * 20.0
    for tm in H.TONEMAPS:
        out = H.tone_map(v, tm, 1000.0 / 203.0)
        assert np.allclose(out * v.max(-1, keepdims=True), v * out.max(-1, keepdims=True), rtol=1e-12)
        assert out.max() <= 1.0 + 1e-15
    assert np.array_equal(H.tone_map(np.zeros((1, 3)), "mobius", 4.0), np.zeros((1, 3)))


# ---------------------------------------------------------------- exact anchors through the whole definition --------------------
@pytest.mark.parametrize("transfer", H.TRANSFERS)
def test_black_and_neutrals_are_exact(transfer):
    for tm in H.TONEMAPS:
        assert np.array_equal(H.decode_px(64, 512, 512, transfer, "limited", tm), [0, 0, 0])
        assert np.array_equal(H.decode_px(0, 512, 512, transfer, "full", tm), [0, 0, 0])
        for rng in H.RANGES:
            Y = np.arange(1024)
            out = H.decode_px(Y, np.full(1024, 512), np.full(1024, 512), transfer, rng, tm)
            assert (out[:, 0] == out[:, 1]).all() and (out[:, 1] == out[:, 2]).all(), (transfer, rng, tm)
            assert (np.diff(out[:, 0].astype(int)) >= 0).all() and out[:, 0].max() == 255


def test_pq_grey_at_203_nits_is_white_under_clip():
    L = (203.0 / 10000.0) ** H.PQ_M1
    n = ((H.PQ_C1 + H.PQ_C2 * L) / (1.0 + H.PQ_C3 * L)) ** H.PQ_M2   # the PQ signal of 203 nits (0.58)
    for rng, code in (("limited", 64 + 876 * n), ("full", 1023 * n)):
        y = int(np.ceil(code))                                        # the first code at or above 203 nits
        assert np.array_equal(H.decode_px(y, 512, 512, "pq", rng, "clip"), [255, 255, 255])
        assert H.decode_px(y - 2, 512, 512, "pq", rng, "clip")[0] < 255
    assert np.array_equal(H.srgb_encode(np.array([0.0, 1.0, H.ENC_THR[0], np.nextafter(H.ENC_THR[0], 0)])), [0, 255, 1, 0])


def test_decode_lays_the_formats_out_as_the_raw_reference_does():
    Hh, W = 5, 7
    p010 = R.random_payload("p010le", 2, Hh, W, 3)
    planar = R.join_planes(*R.split_planes(p010, "p010le", Hh, W), "yuv420p10le")
    a = H.decode(p010, "p010le", Hh, W, "pq")
    assert a.shape == (2, Hh, W, 3) and a.dtype == np.uint8 and np.array_equal(a, H.decode(planar, "yuv420p10le", Hh, W, "pq"))
    assert np.array_equal(H.decode(p010[0], "p010le", Hh, W, "hlg"), H.decode(p010, "p010le", Hh, W, "hlg")[0])
    Y, U, V = R.split_planes(planar, "yuv420p10le", Hh, W)
    assert np.array_equal(a[1, 4, 6], H.decode_px(Y[1, 4, 6], U[1, 2, 3], V[1, 2, 3], "pq"))
    with pytest.raises(ValueError):
        H.decode(p010, "nv12", Hh, W, "pq")


# ---------------------------------------------------------------- the error budget of the device's arithmetic -------------------
_f = np.float32


def _pw(x, e):
    """x^e as the kernel forms it: exp2(e * log2(x)) in float32, 0 at x = 0."""
    with np.errstate(divide="ignore"):
        return np.where(x > 0, np.exp2(_f(e) * np.log2(x)), _f(0))


def device_model(Y, U, V, transfer, rng, tonemap, peak_nits=1000.0, sdr_white=203.0):
    """csrc/yuv_hdr.hip::hdr_px in NumPy float32, operation for operation (every constant is the float64 value rounded once, as
    the host side of the kernel rounds it; no table other than the encoder's).  The hardware's exp2 / log2 / rcp are within about
    1 ulp of NumPy's, so this is a model of the device, not a bit-exact copy: tests/test_hdr_gpu.py holds the device itself."""
    full = rng == "full"
    ys, cs, yo = _f(1.0 / 1023.0 if full else 1.0 / 876.0), _f(1.0 / 1023.0 if full else 1.0 / 896.0), 0 if full else 64
    rv, bu = _f(2.0 * (1.0 - H.KR)), _f(2.0 * (1.0 - H.KB))
    gu, gv = _f(-2.0 * H.KB * (1.0 - H.KB) / H.KG), _f(-2.0 * H.KR * (1.0 - H.KR) / H.KG)
    y = (np.asarray(Y) - yo).astype(_f) * ys
    cb, cr = (np.asarray(U) - 512).astype(_f) * cs, (np.asarray(V) - 512).astype(_f) * cs
    e = [np.clip(y + d, _f(0), _f(1)) for d in (rv * cr, gu * cb + gv * cr, bu * cb)]
    if transfer == "pq":
        gain = _f(10000.0 / sdr_white)
        v = []
        for x in e:
            p = _pw(x, 1.0 / H.PQ_M2)
            num, den = p - _f(H.PQ_C1), _f(H.PQ_C2) - _f(H.PQ_C3) * p
            v.append(gain * _pw(np.maximum(num, _f(0)) * (_f(1) / den), 1.0 / H.PQ_M1))
    else:
        gain, k = _f(1000.0 / sdr_white), _f(1.4426950408889634 / H.HLG_A)
        s = [np.where(x <= _f(0.5), x * x * _f(1.0 / 3.0), (np.exp2((x - _f(H.HLG_C)) * k) + _f(H.HLG_B)) * _f(1.0 / 12.0)) for x in e]
        f = gain * _pw(_f(0.2627) * s[0] + _f(0.6780) * s[1] + _f(0.0593) * s[2], 0.2)
        v = [f * x for x in s]
    P = peak_nits / sdr_white
    kn = 0.75 if tonemap == "mobius" else 1.0  # clip is the same curve with the knee at 1
    a = (1.0 - kn) / (P - 1.0)
    m = np.maximum(v[0], np.maximum(v[1], v[2]))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (np.minimum(m, _f(P)) - _f(kn)) * _f(1.0 / (P - kn))
        t = _f(kn) + _f((1.0 - kn) * (1.0 + a)) * u * (_f(1) / (u + _f(a)))
        sc = np.where(m > _f(kn), t * (_f(1) / m), _f(1))
    x = [c * sc for c in v]
    M = H.gamut_matrix().astype(_f)
    out = []
    for i in range(3):
        j, k2 = (i + 1) % 3, (i + 2) % 3
        # the kernel adds the two difference terms in index order: (M_i,lower, M_i,higher)
        lo, hi = min(j, k2), max(j, k2)
        out.append(x[i] + (M[i, lo] * (x[lo] - x[i]) + M[i, hi] * (x[hi] - x[i])))
    thr = H.ENC_THR.astype(_f)
    assert all(o.dtype == _f for o in out)
    return np.stack([np.searchsorted(thr, np.clip(o, _f(0), _f(1)), side="right") for o in out], -1).astype(np.uint8)


_RANDOM = np.random.default_rng(2100).integers(0, 1024, (4_000_000, 3))


@pytest.mark.parametrize("transfer,rng,tonemap", H.COMBOS)
def test_device_arithmetic_within_one_code_of_the_definition(transfer, rng, tonemap):
    """The bound is one code: every stage is continuous and float32's relative error (1e-6 after the curves' amplification)
    is far below the finest output step, 1 / (255 x 12.92) of full scale at the foot of the sRGB curve, so the arithmetic can only
    move a sample across a rounding boundary.  The share of samples that differ at all is printed (DESIGN §4.10 records it)."""
    worst, shares = 0, []
    for name, t in (("lattice", H.lattice()), ("random", _RANDOM)):
        want = H.decode_px(t[:, 0], t[:, 1], t[:, 2], transfer, rng, tonemap).astype(np.int16)
        got = device_model(t[:, 0], t[:, 1], t[:, 2], transfer, rng, tonemap).astype(np.int16)
        d = np.abs(got - want)
        worst = max(worst, int(d.max()))
        shares.append((name, float((d > 0).mean())))
    print(f"hdr budget {transfer} {rng} {tonemap}: max |model - definition| = {worst} code(s); share of samples off by one: "
          + ", ".join(f"{n} {s:.2e}" for n, s in shares))
    assert worst <= 1


@pytest.mark.parametrize("transfer", H.TRANSFERS)
def test_device_arithmetic_keeps_the_anchors_exact(transfer):
    Y = np.arange(1024)
    c = np.full(1024, 512)
    for rng in H.RANGES:
        for tm in H.TONEMAPS:
            out = device_model(Y, c, c, transfer, rng, tm)
            assert (out[:, 0] == out[:, 1]).all() and (out[:, 1] == out[:, 2]).all()
            assert np.array_equal(device_model(np.array([0 if rng == "full" else 64]), c[:1], c[:1], transfer, rng, tm), [[0, 0, 0]])


def test_other_peaks_and_whites_stay_within_one_code():
    t = np.concatenate([H.lattice(), _RANDOM[:500_000]])
    for transfer, peak, white in (("pq", 4000.0, 203.0), ("pq", 10000.0, 100.0), ("hlg", 1000.0, 100.0), ("pq", 204.0, 203.0)):
        want = H.decode_px(t[:, 0], t[:, 1], t[:, 2], transfer, "limited", "mobius", peak, white).astype(np.int16)
        got = device_model(t[:, 0], t[:, 1], t[:, 2], transfer, "limited", "mobius", peak, white).astype(np.int16)
        assert np.abs(got - want).max() <= 1, (transfer, peak, white)


# ---------------------------------------------------------------- the interface, without a device ------------------------------
def test_abi_symbols_declared_bound_and_null_safe():
    from animal_vision_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert re.search(r"\bint\s+avx_yuv_hdr_to_rgb_u8\s*\(", hdr)
    assert re.search(r"enum\s+avx_transfer\s*\{\s*AVX_TRANSFER_PQ\s*=\s*1\s*,\s*AVX_TRANSFER_HLG\s*=\s*2\s*\}", hdr)
    assert re.search(r"enum\s+avx_tonemap\s*\{\s*AVX_TONEMAP_CLIP\s*=\s*0\s*,\s*AVX_TONEMAP_MOBIUS\s*=\s*1\s*\}", hdr)
    assert _lib.AVX_TRANSFERS == {"pq": 1, "hlg": 2} and _lib.AVX_TONEMAPS == {"clip": 0, "mobius": 1}
    fn = _lib.lib.avx_yuv_hdr_to_rgb_u8
    sig = _lib._SIGS["avx_yuv_hdr_to_rgb_u8"]
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(sig[1]) == 13
    assert [t for t in fn.argtypes if t is ctypes.c_double] == [ctypes.c_double] * 2 and fn.argtypes[10] is ctypes.c_double
    # a NULL context is refused before anything else is looked at
    assert fn(None, 8, None, None, 1, 8, 8, 0, 1, 1, 1000.0, 203.0, None) == _lib.AVX_ERR_INVALID


def test_python_checks_come_before_the_device():
    from animal_vision_amd import yuv

    assert yuv.TRANSFERS == ("pq", "hlg") and yuv.TONEMAPS == ("clip", "mobius")
    assert set(yuv.MATRICES) == {"bt601", "bt709"}
    Hh, W = 4, 4
    buf = np.zeros(R.frame_size("p010le", Hh, W), np.uint8)
    ok = dict(pix_fmt="p010le", transfer="pq")
    bad = [dict(ok, pix_fmt="nv12"), dict(ok, pix_fmt="gray"), dict(ok, pix_fmt="yuv420p"), dict(ok, pix_fmt="yuv420p12le"), dict(ok, transfer="srgb"),
           dict(ok, transfer=None), dict(ok, tonemap="hable"), dict(ok, range="tv"), dict(ok, peak_nits=203.0), dict(ok, peak_nits=100.0),
           dict(ok, sdr_white=0.0), dict(ok, sdr_white=-1.0), dict(ok, peak_nits=float("inf")), dict(ok, peak_nits=float("nan")),
           dict(ok, sdr_white=float("nan")), dict(ok, peak_nits="bright")]
    for kw in bad:  # refused before a context is created: this passes on a machine without a GPU
        with pytest.raises(ValueError):
            yuv.yuv_hdr_to_rgb(buf, Hh, W, **kw)
    with pytest.raises(ValueError):
        yuv.yuv_hdr_to_rgb(buf[:-2], Hh, W, **ok)
    with pytest.raises(TypeError):
        yuv.yuv_hdr_to_rgb(buf.view(np.uint16), Hh, W, **ok)
    with pytest.raises(TypeError):
        yuv.yuv_hdr_to_rgb(buf, Hh, W, pix_fmt="p010le")  # transfer is required
    assert yuv.hdr_codes("yuv444p10le", "hlg", "full", "clip", 4000, 100) == (7, 1, 2, 0, 4000.0, 100.0)
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv(np.zeros((4, 4, 3), np.uint8), pix_fmt="p010le", matrix="bt2020")
    # the fixed-point entry points keep refusing matrix code 2 (host only)
    from animal_vision_amd._lib import AVX_ERR_INVALID, lib

    assert lib.avx_yuv_coefficients_d(2, 0, 10, (ctypes.c_int * 6)(), (ctypes.c_int * 10)()) == AVX_ERR_INVALID


def test_pipeline_refuses_bad_hdr_settings_before_it_touches_the_device():
    from animal_vision_amd.pipeline import FramePipeline

    class Op:  # never reached: the checks come before any allocation
        ctx = None

    with pytest.raises(ValueError, match="transfer"):
        FramePipeline(Op(), 16, 16, transfer="pq")                                          # io_format="rgb"
    with pytest.raises(ValueError, match="transfer"):
        FramePipeline(Op(), 16, 16, io_format="i420", transfer="pq")
    with pytest.raises(ValueError, match="10-bit"):
        FramePipeline(Op(), 16, 16, io_format="yuv", pix_fmt="nv12", transfer="pq")
    with pytest.raises(ValueError, match="transfer"):
        FramePipeline(Op(), 16, 16, io_format="yuv", pix_fmt="p010le", transfer="gamma")
    with pytest.raises(ValueError, match="tonemap"):
        FramePipeline(Op(), 16, 16, io_format="yuv", pix_fmt="p010le", transfer="pq", tonemap="hable")
    with pytest.raises(ValueError, match="peak_nits"):
        FramePipeline(Op(), 16, 16, io_format="yuv", pix_fmt="p010le", transfer="pq", peak_nits=100.0)
    with pytest.raises(ValueError, match="matrix"):
        FramePipeline(Op(), 16, 16, io_format="yuv", pix_fmt="p010le", transfer="pq", out_matrix="bt2020")
    with pytest.raises(ValueError, match="matrix"):
        FramePipeline(Op(), 16, 16, io_format="yuv", pix_fmt="p010le", out_matrix="bt2020")


def test_video_renderer_hdr_arguments(tmp_path):
    from animal_vision_amd.renderers import VideoRenderer

    Hh, W = 4, 6
    src = str(tmp_path / "in.yuv")
    with open(src, "wb") as f:
        f.write(R.random_payload("p010le", 2, Hh, W, 1).tobytes())
    vr = VideoRenderer(read_path=src, write_path=str(tmp_path / "o.yuv"), pix_fmt="p010le", size=(W, Hh), transfer="hlg", peak_nits=4000.0)
    assert (vr.transfer, vr.tonemap, vr.peak_nits, vr.sdr_white, vr.out_matrix) == ("hlg", "mobius", 4000.0, 203.0, "bt709")
    vr.open()
    assert vr.yuv_hw == (Hh, W) and vr.yuv_pix_fmt == "p010le"
    vr.close()
    vr = VideoRenderer(read_path=src, write_path=str(tmp_path / "o2.yuv"), pix_fmt="p010le", size=(W, Hh), matrix="bt709")
    assert vr.transfer is None and vr.tonemap == "mobius" and vr.out_matrix == "bt709" and vr.peak_nits == 1000.0 and vr.sdr_white == 203.0
    assert VideoRenderer(read_path="synthetic:8x8:2").out_matrix == "bt601"
    for kw in (dict(pix_fmt="nv12"), dict(pix_fmt="p010le", transfer="srgb"), dict(pix_fmt="p010le", transfer="pq", tonemap="x"),
               dict(pix_fmt="p010le", transfer="pq", sdr_white=2000.0), dict(pix_fmt="p010le", transfer="pq", out_matrix="bt2020")):
        with pytest.raises(ValueError):
            VideoRenderer(read_path=src, size=(W, Hh), **{"transfer": "pq", **kw})
    with pytest.raises(ValueError):
        VideoRenderer(read_path="in.y4m", transfer="pq")  # not a raw 10-bit source


def test_cli_hdr_flags(capsys):
    from animal_vision_amd.video import parse_args

    base = ["-", "out.yuv", "--species", "Dog", "--size", "3840x2160"]
    a = parse_args(base + ["--pix-fmt", "p010le", "--transfer", "pq"])
    assert (a.transfer, a.tonemap, a.peak_nits, a.sdr_white, a.out_matrix) == ("pq", "mobius", 1000.0, 203.0, None)
    a = parse_args(base + ["--pix-fmt", "yuv420p10le", "--transfer", "hlg", "--matrix", "bt2020", "--tonemap", "clip", "--peak-nits", "4000",
                           "--sdr-white", "100", "--out-matrix", "bt601"])
    assert (a.transfer, a.tonemap, a.peak_nits, a.sdr_white, a.out_matrix) == ("hlg", "clip", 4000.0, 100.0, "bt601")
    a = parse_args(["in.y4m", "out.y4m", "--species", "Dog"])  # Y4M is untouched
    assert a.transfer is None and a.matrix == "bt601" and a.out_matrix is None and a.tonemap == "mobius"
    a = parse_args(base + ["--pix-fmt", "p010le", "--matrix", "bt709", "--out-matrix", "bt601"])
    assert a.transfer is None and a.matrix == "bt709" and a.out_matrix == "bt601"

    def refused(extra, *words):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        err = capsys.readouterr().err
        assert all(w in err for w in words), err

    refused(["--pix-fmt", "nv12", "--transfer", "pq"], "--transfer", "--pix-fmt")
    refused(["--pix-fmt", "gray", "--transfer", "hlg"], "--transfer", "--pix-fmt")
    with pytest.raises(SystemExit):
        parse_args(["in.y4m", "out.y4m", "--species", "Dog", "--transfer", "pq"])
    err = capsys.readouterr().err
    assert "--transfer" in err and "--pix-fmt" in err
    refused(["--pix-fmt", "p010le", "--transfer", "pq", "--matrix", "bt709"], "--matrix", "--transfer")
    refused(["--pix-fmt", "p010le", "--transfer", "pq", "--matrix", "bt601"], "--matrix", "--transfer")
    refused(["--pix-fmt", "p010le", "--matrix", "bt2020"], "bt2020", "--transfer")
    refused(["--pix-fmt", "p010le", "--transfer", "gamma"], "--transfer")
    refused(["--pix-fmt", "p010le", "--transfer", "pq", "--tonemap", "hable"], "--tonemap")
    refused(["--pix-fmt", "p010le", "--transfer", "pq", "--peak-nits", "100"], "--peak-nits", "--sdr-white")
    refused(["--pix-fmt", "p010le", "--transfer", "pq", "--sdr-white", "0"], "--sdr-white")
    refused(["--pix-fmt", "p010le", "--transfer", "pq", "--peak-nits", "nan"], "--peak-nits")
    refused(["--pix-fmt", "p010le", "--transfer", "pq", "--out-matrix", "bt2020"], "--out-matrix")
    refused(["--pix-fmt", "p010le", "--tonemap", "clip"], "--tonemap", "--transfer")
    refused(["--pix-fmt", "p010le", "--peak-nits", "4000"], "--peak-nits", "--transfer")
