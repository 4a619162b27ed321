"""No GPU: the host side of the edge-preserving smoothing in front of the edges -- properties of the yardstick of
tests/_smooth_ref.py in both dtypes (a flat frame and a straight seam are exact fixed points, greys stay chromatically 0, an isolated
outlier moves toward its ground monotonically), the float32 figure that sets the device's bound, check_smooth and the `edges` parser
with every refusal by name, the summary, and the exported symbol with its prototype.

test_float32_figure_that_sets_the_device_bound measures what tests/test_edges_smooth_gpu.py's tolerance rests on: the largest
|float32 restatement - float64 yardstick| over _smooth_ref.CASES, the six frame kinds, the three observers and the three channels, of
the edge values and of the smoothed planes in the observer's metric.  _smooth_ref.F32_FIGURE is that figure rounded up (the figures
and the cases that attain them stand there), and the device is held to 8 x it."""
import ctypes
import os

import numpy as np
import pytest

import _acuity_ref as A
import _edges_ref as E
import _smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOG = ["--observer", "Dog", "--weber", "0.05,0.05"]
IN = "synthetic:64x48:3"


def _observers():
    from animal_vision_amd.metrics import Observer, observer_for

    return [observer_for("Dog", (0.05, 0.05)), observer_for("HoneyBee", (0.13, 0.06, 0.12)), Observer("four", A.FOUR, (0.08,) * 4)]


def _run(frame, obs, channel, smooth, sigma=0.0, step=1, dtype=np.float64, key=None):
    return S.planes_and_values(frame, obs.matrix, obs.weber, obs.floor, E.ACHROMATIC[obs.name], channel, sigma, step, smooth, dtype, key)


def split_frame(H, W, c, left, right, vertical=True):
    f = np.empty((H, W, 3), np.uint8)
    if vertical:
        f[:, :c], f[:, c:] = left, right
    else:
        f[:c], f[c:] = left, right
    return f


# ------------------------------------------------------------------------------------------------ properties of the yardstick
def test_a_flat_frame_is_an_exact_fixed_point():
    flat = np.stack([np.broadcast_to(np.array(c, np.uint8), (9, 13, 3)) for c in ((200, 60, 60), (0, 0, 0), (255, 255, 255))])
    for obs in _observers():
        for ch in E.CHANNELS:
            for dtype in (np.float64, np.float32):
                before = _run(flat, obs, ch, (1, 0.5, 0), dtype=dtype)[0]
                for smooth in S.SETTINGS:
                    planes, values, _ = _run(flat, obs, ch, smooth, dtype=dtype)
                    assert planes.tobytes() == before.tobytes() and not values.any(), (obs.name, ch, smooth, dtype)


def test_greys_stay_chromatically_zero():
    g = np.stack(A.grey_frames(12, 20))
    for obs in _observers():
        K = obs.n_receptors
        for ch in ("chromatic", "either"):
            for sigma in (0.0, 1.0):
                for dtype in (np.float64, np.float32):
                    for smooth in ((1, 0.5, 2), (5, 0.33, 3), (2, 1.0, 1)):
                        f = _run(g, obs, ch, smooth, sigma, dtype=dtype)[2]
                        assert all(np.array_equal(f[..., 0], f[..., i]) for i in range(1, K)), (obs.name, ch, sigma, smooth)
                        assert not S.edge_values(f, obs.weber, E.ACHROMATIC[obs.name][1], "chromatic", 1, dtype).any()
                assert _run(g, obs, "achromatic", (2, 0.5, 1), sigma)[1].any()


@pytest.mark.parametrize("vertical", [True, False])
def test_a_straight_seam_is_an_exact_fixed_point_at_keep_up_to_a_half(vertical):
    """Two flat colours: at KEEP <= 0.5 at least m pixels of every window are the pixel's own colour -- its side of the seam holds
    more than half of the window when the seam is at least R from the frame's sides --, so t = 0, only they weigh and nothing moves."""
    H, W, c = 24, 28, 11
    f = split_frame(H, W, c, (200, 60, 60), (60, 200, 60), vertical)
    for obs in _observers():
        for ch in E.CHANNELS:
            for dtype in (np.float64, np.float32):
                before, v0, _ = _run(f, obs, ch, (1, 0.5, 0), dtype=dtype)
                assert v0.any()
                for R in range(1, 6):
                    for keep in (0.5, 0.25):
                        planes, values, _ = _run(f, obs, ch, (R, keep, 3), dtype=dtype)
                        assert planes.tobytes() == before.tobytes() and values.tobytes() == v0.tobytes(), (obs.name, ch, R, keep, dtype)
    # and above a half the seam does move
    assert _run(f, _observers()[0], "either", (3, 1.0, 1))[0].tobytes() != _run(f, _observers()[0], "either", (3, 1.0, 0))[0].tobytes()


def test_an_isolated_outlier_moves_toward_its_ground_monotonically():
    f = np.full((9, 9, 3), 120, np.uint8)
    f[4, 4] = (220, 80, 120)
    for obs in _observers():
        lw = E.ACHROMATIC[obs.name][1]
        for dtype in (np.float64, np.float32):
            far = []
            for it in range(4):
                full = _run(f, obs, "either", (1, 0.5, it), dtype=dtype)[2]
                far.append(float(E.pair_value(full[4, 4], full[0, 0], obs.weber, lw, "either", dtype)))
            print(f"outlier {obs.name} {dtype.__name__}: " + ", ".join(f"{d:.4f}" for d in far))
            assert far[0] > 1 and all(a > b for a, b in zip(far, far[1:])) and far[3] < 0.1 * far[0], (obs.name, far)


def test_rank_table_and_cases():
    assert list(S.rank_table(0.5)[:6]) == [0, 1, 1, 2, 2, 3] and S.rank_table(1.0)[121] == 121 and set(S.rank_table(0.01)[1:]) == {1, 2}
    assert S.rank_table(0.01)[100] == 1 and S.rank_table(0.33)[121] == 40
    assert S.SETTINGS == ((1, 0.5, 2), (3, 0.3, 1), (5, 0.33, 3), (2, 1.0, 1), (5, 0.01, 1))
    assert list(S.CASES) == [(1, 1), (1, 9), (2, 3), (5, 7), (16, 16), (33, 70), (70, 130)]
    classes = [[(1, 1)], [(1, 9)], [(2, 3), (5, 7)], [(16, 16)], [(33, 70), (70, 130)]]
    for cl in classes:  # every setting meets every size class
        assert {c[0] for size in cl for c in S.CASES[size]} == set(S.SETTINGS), cl
    runs = {c[1:] for cases in S.CASES.values() for c in cases}
    assert {s for s, _ in runs} == {0.0, 1.0} and {d for _, d in runs} == {1, 8}


# ------------------------------------------------------------------------------------------------ the float32 figure
def test_float32_figure_that_sets_the_device_bound():
    worst_v, worst_p = (-1.0, ()), (-1.0, ())
    largest = 0.0
    for (H, W), cases in S.CASES.items():
        f = E.frames(H, W)
        for smooth, sigma, D in cases:
            for obs in _observers():
                lw = E.ACHROMATIC[obs.name][1]
                for ch in E.CHANNELS:
                    p64, v64, _ = _run(f, obs, ch, smooth, sigma, D, np.float64, key=(H, W))
                    p32, v32, _ = _run(f, obs, ch, smooth, sigma, D, np.float32, key=(H, W))
                    assert p32.dtype == v32.dtype == np.float32 and p64.dtype == v64.dtype == np.float64 and v64.shape == (len(E.KINDS), H, W)
                    dv = float(np.abs(v32.astype(np.float64) - v64).max())
                    dp = float(S.plane_error(p32, p64, obs.n_receptors, obs.weber, lw, ch).max())
                    what = (obs.name, ch, H, W, smooth, sigma, D)
                    worst_v, worst_p = max(worst_v, (dv, what)), max(worst_p, (dp, what))
                    largest = max(largest, float(v64.max()))
                    print(f"smooth float32 restatement {H}x{W} {smooth} sigma {sigma} step {D} {obs.name} {ch}: values {dv:.3e}, planes {dp:.3e}, "
                          f"largest value {v64.max():.3f}")
    print(f"the float32 figure: values {worst_v[0]:.3e} at {worst_v[1]}, planes {worst_p[0]:.3e} at {worst_p[1]}; largest value {largest:.1f}; "
          f"F32_FIGURE {S.F32_FIGURE:g}, the device's bound {S.BOUND:g}")
    assert worst_v[0] <= S.F32_FIGURE and worst_p[0] <= S.F32_FIGURE
    assert S.BOUND == 8 * S.F32_FIGURE


# ------------------------------------------------------------------------------------------------ options, the parser, the summary
def test_check_smooth():
    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import check_edges_options, check_smooth, observer_for

    assert check_smooth(None) is None
    d = check_smooth((3, 0.5))
    assert isinstance(d, _lib.SmoothDesc) and (d.struct_size, d.radius, d.keep, d.iterations) == (24, 3, 0.5, 1)
    d = check_smooth([5, 1, 0])
    assert (d.radius, d.keep, d.iterations) == (5, 1.0, 0) and check_smooth((1, 1e-9, 8)).iterations == 8
    nan = float("nan")
    for bad, words in (((0, 0.5), "smooth radius must be a whole number of pixels from 1 to 5"), ((6, 0.5), "smooth radius"), ((1.5, 0.5), "smooth radius"),
                       ((True, 0.5), "smooth radius"), ((3, 0.0), "smooth keep must be a number above 0 and at most 1"), ((3, 1.01), "smooth keep"),
                       ((3, nan), "smooth keep"), ((3, "half"), "smooth keep"), ((3, 0.5, -1), "smooth iterations must be a whole number from 0 to 8"),
                       ((3, 0.5, 9), "smooth iterations"), ((3, 0.5, 1.0), "smooth iterations"), ((3,), r"smooth must be \(radius, keep\)"),
                       ((3, 0.5, 1, 1), r"smooth must be \(radius, keep\)"), (3, r"smooth must be \(radius, keep\)")):
        with pytest.raises(ValueError, match=words):
            check_smooth(bad)
        with pytest.raises(ValueError, match=words):
            check_edges_options(observer_for("Dog", (0.05, 0.05)), smooth=bad)
    assert len(check_edges_options(observer_for("Dog", (0.05, 0.05)), smooth=(3, 0.5))) == 4  # what it returned before


def test_metrics_refuse_a_bad_smooth_before_the_device(monkeypatch):
    from animal_vision_amd import metrics

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(metrics, "get_context", no_device)
    dog = metrics.observer_for("Dog", (0.05, 0.05))
    f = np.zeros((12, 14, 3), np.uint8)
    for fn in (metrics.receptor_edges, metrics.receptor_edges_map, metrics.receptor_edges_values, metrics.receptor_smooth_planes):
        for bad, words in (((0, 0.5), "smooth radius"), ((3, 2.0), "smooth keep"), ((3, 0.5, 9), "smooth iterations"), ("3:0.5", "smooth must be")):
            with pytest.raises(ValueError, match=words):
                fn(f, dog, smooth=bad)
        with pytest.raises(AssertionError, match="the device was asked for"):  # a good one does reach the device
            fn(f, dog, smooth=(3, 0.5, 2))
    with pytest.raises(ValueError, match="smooth must be"):
        metrics.receptor_smooth_planes(f, dog, smooth=None)

    class Buf:
        ptr, nbytes = 0, 12 * 14 * 3

    class Rec:
        ptr, nbytes = 0, metrics.DELTA_E_RECORD_BYTES

    with pytest.raises(ValueError, match="smooth radius"):
        metrics.receptor_edges_launch(None, Buf(), 1, 12, 14, None, Rec(), observer=dog, smooth=(9, 0.5))
    with pytest.raises(ValueError, match="d_planes takes the smoothed planes"):
        metrics.receptor_edges_launch(None, Buf(), 1, 12, 14, None, Rec(), observer=dog, d_planes=Buf())
    with pytest.raises(ValueError, match="the planes need 1344"):
        metrics.receptor_edges_launch(None, Buf(), 1, 12, 14, None, Rec(), observer=dog, smooth=(1, 0.5), d_planes=Buf())
    assert metrics.edges_planes(dog, "chromatic") == 2 and metrics.edges_planes(dog, "achromatic") == 1 and metrics.edges_planes(dog, "either") == 3


def _error(capsys, argv):
    from animal_vision_amd import edges

    with pytest.raises(SystemExit) as e:
        edges.parse_args(argv)
    assert e.value.code == 2, argv
    return capsys.readouterr().err


def test_the_parser_and_the_summary(capsys):
    from animal_vision_amd import edges

    a = edges.parse_args([IN] + DOG + ["--smooth", "3:0.5:2"])
    assert a.smooth == (3, 0.5, 2) and edges.describe(a) == "Dog, weber 0.05,0.05, floor 0.001, smooth 3:0.5x2, step 1"
    a = edges.parse_args([IN] + DOG + ["--achromatic", "1:0.1", "--acuity", "species", "--smooth", "5:1"])
    assert a.smooth == (5, 1.0, 1)
    assert edges.describe(a) == "Dog, weber 0.05,0.05, floor 0.001, achromatic 1:0.1, acuity 3.5 px, smooth 5:1x1, step 1"
    # without --smooth the namespace and the summary are what they were
    a = edges.parse_args([IN] + DOG + ["--achromatic", "1:0.1", "--acuity", "species"])
    assert "smooth" not in vars(a) and edges.describe(a) == "Dog, weber 0.05,0.05, floor 0.001, achromatic 1:0.1, acuity 3.5 px, step 1"
    assert sorted(vars(edges.parse_args([IN] + DOG + ["--smooth", "1:0.5"]))) == sorted(list(vars(a)) + ["smooth"])
    assert "--smooth RADIUS:KEEP[:ITERATIONS]" in edges.build_parser().format_help() and "RNL ranked filter" in edges.__doc__
    for bad in ("3", "3:0.5:2:1", "a:0.5", "3:half", "3:0.5:x", "3.5:0.5", ""):
        assert "--smooth: RADIUS:KEEP[:ITERATIONS]" in _error(capsys, [IN] + DOG + [f"--smooth={bad}"]), bad
    for bad in ("0:0.5", "6:0.5", "-1:0.5"):
        assert "--smooth: RADIUS must be 1..5" in _error(capsys, [IN] + DOG + [f"--smooth={bad}"]), bad
    for bad in ("3:0", "3:1.5", "3:-0.5", "3:nan", "3:inf"):
        assert "--smooth: KEEP must be above 0 and at most 1" in _error(capsys, [IN] + DOG + [f"--smooth={bad}"]), bad
    for bad in ("3:0.5:0", "3:0.5:9", "3:0.5:-1"):
        assert "--smooth: ITERATIONS must be 1..8" in _error(capsys, [IN] + DOG + [f"--smooth={bad}"]), bad


def test_the_launch_gets_the_smooth(monkeypatch, capsys):
    from animal_vision_amd import edges
    from animal_vision_amd.metrics import DeltaE

    h = np.zeros(256, np.int64)
    h[0] = 24
    monkeypatch.setattr(edges, "stream_records", lambda args, info, fmt=None: iter([(None, DeltaE(h, 0.0, 0.0, 0, 0, 0))]))
    assert edges.main([IN] + DOG + ["--smooth", "3:0.5:2"]) == 0
    assert "mean RNL edges (Dog, weber 0.05,0.05, floor 0.001, smooth 3:0.5x2, step 1) 0.000000" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the symbol
def test_symbol_is_declared_exported_and_bound():
    from animal_vision_amd import _lib

    fn = _lib.lib.avx_receptor_edges_smooth_u8
    assert "avx_receptor_edges_smooth_u8" in _lib._SIGS and fn.restype is ctypes.c_int and len(fn.argtypes) == 19
    assert fn.argtypes[5] is ctypes.POINTER(_lib.ReceptorDesc) and fn.argtypes[6] is ctypes.POINTER(_lib.LuminanceDesc)
    assert fn.argtypes[8] is ctypes.c_double and fn.argtypes[10] is ctypes.POINTER(_lib.SmoothDesc) and fn.argtypes[12] is ctypes.c_float
    assert fn(None, None, 1, 16, 16, None, None, 0, 0.0, 1, None, 0, 10.0, 1.0, None, None, None, None, None) == _lib.AVX_ERR_INVALID  # a NULL context first
    assert _lib.lib.avx_abi_version() == 1 and len(_lib.lib.avx_receptor_edges_u8.argtypes) == 17
    assert [(n, t) for n, t in _lib.SmoothDesc._fields_] == [("struct_size", ctypes.c_uint32), ("radius", ctypes.c_int32), ("keep", ctypes.c_double),
                                                             ("iterations", ctypes.c_int32), ("reserved", ctypes.c_uint32)]
    assert ctypes.sizeof(_lib.SmoothDesc) == 24 and _lib.SmoothDesc.keep.offset == 8 and _lib.SmoothDesc.iterations.offset == 16
    hdr = open(os.path.join(ROOT, "include", "avx.h")).read()
    assert ("int avx_receptor_edges_smooth_u8(avx_ctx* ctx, const uint8_t* hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,\n"
            "                                 const avx_luminance_desc* lum, int channel, double sigma, int step, const avx_smooth_desc* smooth, int mode,\n"
            "                                 float gain, float threshold, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out, float* planes_out,\n"
            "                                 void* stream);") in hdr
    assert ("typedef struct avx_smooth_desc {\n    uint32_t struct_size;  /* sizeof(avx_smooth_desc) */\n    int32_t radius;        /* R */\n"
            "    double keep;           /* KEEP */\n    int32_t iterations;    /* ITER */\n    uint32_t reserved;     /* not read */\n} avx_smooth_desc;") in hdr
    assert "#define AVX_ABI_VERSION 1" in hdr and "m = ceil(KEEP N)" in hdr
    csrc = os.path.join(ROOT, "animal-vision_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "receptor_smooth.hip" in mk and "receptor_edges_common.h" in mk
    src = open(os.path.join(csrc, "receptor_smooth.hip")).read()
    assert '#include "receptor_edges_common.h"' in src and "Rnl<K>" in src and "pair_class" not in src and "from_contrasts(" in src
    assert "de_record_share(" in src and "de_px_panels(" in src and "atomicAdd(" not in src
