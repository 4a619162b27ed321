"""No GPU: the host side of the S-CIELAB colour difference -- the yardstick of tests/_scielab_ref.py against its own
definition (taps, weights, flat frames, the checkerboard no viewer resolves, locality, frames below the support), `deltae --ppd` in the
parser, the argument checks of metrics.scielab* that need no device, the exported symbol with its prototype, and the command's
bookkeeping with the device loop stubbed."""
import ctypes
import os

import numpy as np
import pytest

import _deltae_ref as E
import _scielab_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("ppd", [2, 9, 22.5, 60, 128])
def test_taps_are_symmetric_normalised_and_of_the_stated_length(ppd):
    import math

    for channel in S.TERMS:
        for _, spread in channel:
            g = S.taps(spread, ppd)
            assert len(g) == 2 * math.ceil(ppd / 2) + 1 == 2 * S.radius(ppd) + 1
            assert np.array_equal(g, g[::-1]) and abs(g.sum() - 1.0) <= 1e-15 and (g > 0).all() and g.argmax() == len(g) // 2
    assert (S.radius(2), S.radius(9), S.radius(22.5), S.radius(60), S.radius(128)) == (1, 5, 12, 30, 64)


def test_channel_weights_sum_to_one():
    for c in range(3):
        assert abs(S.weights(c).sum() - 1.0) <= 1e-15 and len(S.weights(c)) == len(S.TERMS[c])
    assert S.weights(0)[2] < 0  # the wide luminance term is subtracted


def test_flat_frames_give_the_plain_delta_e():
    """Filters of unit sum leave a flat frame alone: what remains is P, its inverse and the white scaling against _deltae_ref's Lab."""
    worst = 0.0
    for x, y in (((200, 30, 90), (10, 220, 130)), ((0, 0, 255), (255, 255, 0)), ((12, 12, 12), (14, 11, 12)), ((255, 255, 255), (0, 0, 0))):
        a, b = np.empty((9, 11, 3), np.uint8), np.empty((9, 11, 3), np.uint8)
        a[...], b[...] = x, y
        want = E.ciede2000(E.lab(a), E.lab(b))
        for ppd in (2, 9, 60):
            worst = max(worst, float(np.abs(S.scielab(a, b, ppd) - want).max()))
    assert worst <= 1e-12, worst


def test_one_pixel_checkerboard_is_not_seen_at_60_ppd():
    a, b = S.checkerboard()
    plain = float(E.delta_e(a, b).mean())
    v = S.scielab(a, b, 60)
    assert 11.8 < plain < 11.85 and v.mean() < 0.25 * plain and v[30:-30, 30:-30].max() < 0.05, (plain, v.mean())
    assert 5.0 < S.scielab(a, b, 30).mean() < 5.25
    assert S.scielab(a, b, 9).mean() > plain  # the chroma channels blur, the luminance channel does not: the method, not a bug


def test_a_changed_pixel_reaches_exactly_its_support():
    a = S.frame("noise", 40, 40, 1)
    b = a.copy()
    b[20, 20] ^= 0x55
    v = S.scielab(a, b, 9)
    R = S.radius(9)
    hit = np.zeros((40, 40), bool)
    hit[20 - R:20 + R + 1, 20 - R:20 + R + 1] = True
    assert (v != 0).sum() == (2 * R + 1) ** 2 == 121 and np.array_equal(v != 0, hit)
    assert (S.scielab(a, a.copy(), 9) == 0).all()


def test_frames_below_the_support_run():
    a = S.frame("noise", 5, 7, 2)
    v = S.scielab(a, S.jitter(a, 3), 60)
    assert v.shape == (5, 7) and np.isfinite(v).all() and v.max() > 0
    assert S.scielab(a[:1, :1], a[1:2, 1:2], 128).shape == (1, 1)


# ------------------------------------------------------------------------------------------------ the parser
def _error(capsys, argv):
    from animal_vision_amd import deltae

    with pytest.raises(SystemExit) as e:
        deltae.parse_args(argv)
    assert e.value.code == 2, argv
    return capsys.readouterr().err


def test_ppd_in_the_parser(capsys):
    from animal_vision_amd import deltae

    assert deltae.parse_args(["a.npy", "b.npy"]).ppd is None and deltae.parse_args(["a.npy", "b.npy", "o.y4m"]).ppd is None
    a = deltae.parse_args(["a.npy", "b.npy", "--ppd", "60"])  # it belongs to the statistics: valid without OUT
    assert a.ppd == 60.0 and a.out is None and (a.mode, a.gain, a.threshold, a.layout) == ("heat", 10.0, 1.0, "map")
    a = deltae.parse_args(["a.npy", "b.npy", "o.npy", "--ppd", "22.5", "--mode", "plain", "--layout", "side", "--max-p95", "2"])
    assert (a.ppd, a.out, a.mode, a.layout, a.max_p95) == (22.5, "o.npy", "plain", "side", 2.0)
    assert deltae.parse_args(["a", "b", "--ppd", "2"]).ppd == 2.0 and deltae.parse_args(["a", "b", "--ppd", "128"]).ppd == 128.0
    for bad in ("1.9", "128.5", "nan", "inf", "0", "-60"):
        err = _error(capsys, ["a.npy", "b.npy", f"--ppd={bad}"])
        assert "--ppd" in err and "ppd must be a finite number from 2 to 128" in err, bad
    assert "--ppd" in deltae.build_parser().format_help() and "tan 1 degree" in deltae.__doc__
    assert deltae.CSV_HEADER == "frame,de_mean,de_p50,de_p95,de_max,x,y,beyond"


# ------------------------------------------------------------------------------------------------ metrics.scielab* without a device
def test_scielab_refuses_bad_arguments_before_the_device(monkeypatch):
    from animal_vision_amd import metrics

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    a = np.zeros((12, 14, 3), np.uint8)
    with pytest.raises(ValueError, match=r"\(12, 14, 3\).*\(12, 15, 3\)"):
        metrics.scielab_map(a, np.zeros((12, 15, 3), np.uint8), ppd=60)
    with pytest.raises(ValueError, match=r"uint8.*float32"):
        metrics.scielab(a, a.astype(np.float32), ppd=60)
    with pytest.raises(ValueError, match="uint8"):
        metrics.scielab_values(a.astype(np.uint16), a, ppd=60)
    for ppd in (1.9, 128.5, float("nan"), float("inf"), 0, -3, "60", None, True):
        for call in (lambda: metrics.scielab(a, a, ppd=ppd), lambda: metrics.scielab_map(a, a, ppd=ppd), lambda: metrics.scielab_values(a, a, ppd=ppd)):
            with pytest.raises(ValueError, match="ppd must be a finite number from 2 to 128"):
                call()
    with pytest.raises(TypeError):
        metrics.scielab(a, a)  # ppd has no default
    for kw, msg in ((dict(mode="abs"), "mode must be one of heat, plain"), (dict(layout="top"), "layout must be one of map, side"),
                    (dict(threshold=-1.0), "threshold must be finite and at least 0"), (dict(threshold=float("nan")), "threshold must be finite"),
                    (dict(gain=0), "gain must be above 0 and at most 255"), (dict(gain=255.5), "gain must be above 0"), (dict(gain=True), "gain must be above 0")):
        with pytest.raises(ValueError, match=msg):
            metrics.scielab_map(a, a, ppd=60, **kw)
    with pytest.raises(ValueError, match="threshold must be finite and at least 0"):
        metrics.scielab(a, a, ppd=60, threshold=-1)
    for call in (lambda: metrics.scielab(a, a, ppd=2), lambda: metrics.scielab_values(a, a, ppd=128.0),
                 lambda: metrics.scielab_map(a, a, ppd=22.5, mode="plain", gain=255, threshold=0, layout="side")):
        with pytest.raises(AssertionError, match="the device was asked for"):
            call()
    assert metrics.check_ppd(60) == 60.0 and isinstance(metrics.check_ppd(60), float) and metrics.check_ppd(np.float32(22.5)) == 22.5

    class Buf:
        ptr, nbytes = 0, 12 * 14 * 3

    class Rec:
        ptr, nbytes = 0, metrics.DELTA_E_RECORD_BYTES

    with pytest.raises(ValueError, match="side frames need"):
        metrics.scielab_launch(None, Buf(), Buf(), 1, 12, 14, Buf(), Rec(), ppd=60, layout="side")
    with pytest.raises(ValueError, match="records need"):
        metrics.scielab_launch(None, Buf(), Buf(), 1, 12, 14, None, Buf(), ppd=60)
    with pytest.raises(ValueError, match="the values of 1 frames need"):
        metrics.scielab_launch(None, Buf(), Buf(), 1, 12, 14, None, Rec(), ppd=60, d_float=Buf())
    with pytest.raises(ValueError, match="ppd must be"):
        metrics.scielab_launch(None, Buf(), Buf(), 1, 12, 14, None, Rec(), ppd=1)
    with pytest.raises(ValueError):
        metrics.scielab_launch(None, Buf(), Buf(), 17, 12, 14, None, Rec(), ppd=60)
    with pytest.raises(ValueError, match="need"):
        metrics.scielab_launch(None, Buf(), Buf(), 2, 12, 14, None, Rec(), ppd=60)  # inputs of one frame, two asked for


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib

    fn = _lib.lib.avx_scielab_u8
    assert "avx_scielab_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    assert fn.argtypes[6] is ctypes.c_double and fn.argtypes[8] is ctypes.c_float and fn.argtypes[9] is ctypes.c_float
    assert fn(None, None, None, 1, 16, 16, 60.0, 0, 10.0, 1.0, 0, None, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context is refused first
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert ("int avx_scielab_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, double ppd, int mode, float gain,\n"
            "                   float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream);") in hdr
    assert "#define AVX_ABI_VERSION 1" in hdr
    mk = open(os.path.join(ROOT, "animal-vision_amd", "csrc", "Makefile")).read()
    assert "scielab.hip" in mk and "delta_e_common.h" in mk
    # one dE00 for both kernels: neither file carries its own copy
    for name in ("delta_e.hip", "scielab.hip"):
        src = open(os.path.join(ROOT, "animal-vision_amd", "csrc", name)).read()
        assert '#include "delta_e_common.h"' in src and "float ciede2000(" not in src and "float lab_f(" not in src, name


# ------------------------------------------------------------------------------------------------ the command, the device loop stubbed
def _records():
    from animal_vision_amd.metrics import DeltaE

    h0 = np.zeros(256, np.int64)
    h0[0] = 24
    h1 = np.zeros(256, np.int64)
    h1[0], h1[4], h1[20] = 12, 10, 2
    return [DeltaE(h0, 0.0, 0.0, 0, 0, 0), DeltaE(h1, 48.0, 10.25, 5, 2, 12), DeltaE(h1, 36.0, 10.25, 1, 1, 12)]


def _run(monkeypatch, capsys, items, argv):
    from animal_vision_amd import deltae

    seen = {}

    def stub(args, info, fmt=None):
        seen["ppd"] = args.ppd
        info["hw"] = (4, 6)
        yield from items

    monkeypatch.setattr(deltae, "stream_records", stub)
    status = deltae.main(argv)
    cap = capsys.readouterr()
    return status, cap.out, cap.err, seen["ppd"]


def test_command_bookkeeping_with_ppd(monkeypatch, capsys):
    none = [(None, r) for r in _records()]
    rows = ["frame,de_mean,de_p50,de_p95,de_max,x,y,beyond", "0,0.000000,0.500000,0.500000,0.000000,0,0,0", "1,2.000000,0.500000,10.500000,10.250000,5,2,12",
            "2,1.500000,0.500000,10.500000,10.250000,1,1,12"]
    status, stdout, err, ppd = _run(monkeypatch, capsys, none, ["a.npy", "b.npy", "--ppd", "60"])
    assert status == 0 and ppd == 60.0 and stdout.splitlines() == rows
    assert "deltae: 3 frames, mean S-CIELAB dE (ppd 60) 1.166667, largest dE 10.250000 (frame 1, pixel x 5 y 2), 24 pixels beyond 1," in err
    status, stdout, err, ppd = _run(monkeypatch, capsys, none, ["a.npy", "b.npy", "--ppd", "22.5", "--threshold", "3"])
    assert status == 0 and ppd == 22.5 and "mean S-CIELAB dE (ppd 22.5) 1.166667" in err and "24 pixels beyond 3," in err
    status, stdout, err, ppd = _run(monkeypatch, capsys, none, ["a.npy", "b.npy"])
    assert status == 0 and ppd is None and "deltae: 3 frames, mean dE 1.166667, largest dE" in err and "S-CIELAB" not in err
    # the limits and their statuses are those of the plain command
    for argv, line in ((["--max-mean", "1.75"], "deltae: frame 1: mean dE 2.000000 is above --max-mean 1.75"),
                       (["--max-p95", "10"], "deltae: frame 1: 95th percentile dE 10.500000 is above --max-p95 10"),
                       (["--max-de", "10"], "deltae: frame 1: largest dE 10.250000 (pixel x 5 y 2) is above --max-de 10")):
        status, stdout, err, _ = _run(monkeypatch, capsys, none, ["a.npy", "b.npy", "--ppd", "60"] + argv)
        assert status == 1 and line in err and len(stdout.splitlines()) == 4, argv
    status, _, err, _ = _run(monkeypatch, capsys, none, ["a.npy", "b.npy", "--ppd", "60", "--max-mean", "2", "--max-p95", "10.5", "--max-de", "10.25"])
    assert status == 0 and "frame 1:" not in err


def test_stream_records_picks_the_launch_by_ppd(monkeypatch):
    from animal_vision_amd import deltae

    calls = []
    monkeypatch.setattr(deltae, "delta_e_launch", lambda *a, **k: calls.append(("plain", k)))
    monkeypatch.setattr(deltae, "scielab_launch", lambda *a, **k: calls.append(("scielab", k)))
    monkeypatch.setattr(deltae, "stream_map_pairs", lambda args, info, name, fmt, launch, nbytes, read: launch(None, None, None, 1, 4, 6, None, None, "s"))
    deltae.stream_records(deltae.parse_args(["a.npy", "b.npy"]), {})
    deltae.stream_records(deltae.parse_args(["a.npy", "b.npy", "--ppd", "30", "--threshold", "2"]), {})
    assert [c[0] for c in calls] == ["plain", "scielab"]
    assert "ppd" not in calls[0][1] and calls[1][1] == dict(ppd=30.0, mode="heat", gain=10.0, threshold=2.0, layout="map", stream="s")
