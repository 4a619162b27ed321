"""GPU: the plane-metrics kernels (csrc/plane_metrics.hip) against the float64 definition of tests/_plane_metrics_ref.py,
and compare --planes yuv end to end.  Small frames only: the sizes are where plane geometry and tiling can go wrong (T = the
kernel's 32 x 32 tile of window positions): (11, 11) leaves no chroma window position, (21, 22) and (22, 21) exactly one in 4:2:0
(odd sizes, so ceil matters), (2T + 21, 2T + 19) makes the 4:2:0 chroma plane straddle a tile edge.

SSIM bound: 1e-5 absolute per frame and plane at both depths, the bound of tests/test_metrics_gpu.py for this quantity; the reference
is the float64 definition itself.  In a float32 emulation every pair kind but flat max against max - 1 stays below 5e-7; that pair is
what separates a careless 10-bit form (3.3e-5 with a fixed centre, 2.0e-4 uncentred) and an uncentred 8-bit form (6.7e-5) from a
correct one."""
import math

import numpy as np
import pytest

import _plane_metrics_ref as P
import _rawyuv_ref as Y
from animal_vision_amd.metrics import PlaneMetrics, plane_metrics  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu

T = 32
FORMATS = ["yuv420p", "nv12", "yuv422p", "yuv444p", "gray", "yuv420p10le", "yuv422p10le", "yuv444p10le", "p010le"]
SIZES = [(10, 40), (11, 11), (21, 22), (22, 21), (37, 53), (T + 10, T + 10), (T + 11, T + 9), (2 * T + 21, 2 * T + 19), (270, 480)]
SSIM_TOL = 1e-5
_cache = {}
_worst = {8: 0.0, 10: 0.0}


def _pairs(fmt, H, W):
    """The six pair kinds and one more of independent noise as payloads of `fmt`, with the reference's histogram and SSIM of each;
    computed once."""
    key = (fmt, H, W)
    if key not in _cache:
        r = Y.random_payload(fmt, 2, H, W, seed=H * 1000 + W)
        pairs = P.six_pairs(fmt, H, W, seed=H + W) + [("random", r[0], r[1])]
        a, b = np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs])
        a.setflags(write=False), b.setflags(write=False)
        _cache[key] = ([p[0] for p in pairs], a, b, [P.abs_hist(x, y, fmt, H, W) for x, y in zip(a, b)],
                       [P.ssim(x, y, fmt, H, W) for x, y in zip(a, b)])
    return _cache[key]


def _same(m, n):
    return m.depth == n.depth and np.array_equal(m.abs_hist, n.abs_hist) and np.array(m.ssim).tobytes() == np.array(n.ssim).tobytes()


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_histogram_exact_and_ssim_within_bound(fmt, H, W):
    names, a, b, hists, ssims = _pairs(fmt, H, W)
    depth, counts = Y.depth_of(fmt), P.plane_samples(fmt, H, W)
    got = plane_metrics(a, b, pix_fmt=fmt, H=H, W=W)
    assert len(got) == len(names)
    worst = 0.0
    for name, m, h, s in zip(names, got, hists, ssims):
        assert m.depth == depth and m.plane_samples == counts and m.planes == ("y" if fmt == "gray" else "yuv")
        assert np.array_equal(m.abs_hist, h[:, : 1 << depth]), (name, fmt, H, W)
        assert m.sse == tuple(P.sse_from_hist(h))
        for p in range(3):
            assert math.isnan(m.ssim[p]) == math.isnan(s[p]), (name, fmt, H, W, p, m.ssim[p], s[p])
            if not math.isnan(s[p]):
                worst = max(worst, abs(m.ssim[p] - s[p]))
    _worst[depth] = max(_worst[depth], worst)
    print(f"plane metrics {fmt} {H}x{W}: largest SSIM deviation {worst:.3e} (so far at {depth} bits: {_worst[depth]:.3e})")
    for name, m, s in zip(names, got, ssims):
        for p in range(3):
            if not math.isnan(s[p]):
                assert abs(m.ssim[p] - s[p]) <= SSIM_TOL, (name, fmt, H, W, p, m.ssim[p], s[p])
    # with_ssim = 0: the same histograms, NaN
    for name, m, h in zip(names, plane_metrics(a, b, pix_fmt=fmt, H=H, W=W, ssim=False), hists):
        assert np.array_equal(m.abs_hist, h[:, : 1 << depth]) and all(math.isnan(v) for v in m.ssim), (name, fmt, H, W)


@pytest.mark.parametrize("planar,semi", [("yuv420p", "nv12"), ("yuv420p10le", "p010le")])
def test_layouts_agree(planar, semi):
    for H, W in ((21, 22), (37, 53), (2 * T + 21, 2 * T + 19)):
        a = Y.random_payload(planar, 3, H, W, seed=H)
        b = Y.join_planes(*Y.split_planes(a, planar, H, W), semi)
        counts = P.plane_samples(planar, H, W)
        for x, y, fx, fy in ((a, b, planar, semi), (b, a, semi, planar)):
            for ssim in (True, False):
                for m in plane_metrics(x, y, pix_fmt=fx, pix_fmt_b=fy, H=H, W=W, ssim=ssim):
                    assert tuple(int(v) for v in m.abs_hist[:, 0]) == counts and m.max_abs == 0 and m.psnr == math.inf
                    assert m.ssim == (1.0, 1.0, 1.0) if ssim else all(math.isnan(v) for v in m.ssim)
        # a differing pair: the record does not depend on the layout either side is stored in
        c = Y.random_payload(planar, 3, H, W, seed=H + 1)
        c2 = Y.join_planes(*Y.split_planes(c, planar, H, W), semi)
        want = plane_metrics(a, c, pix_fmt=planar, H=H, W=W)
        for x, y, fx, fy in ((a, c2, planar, semi), (b, c, semi, planar), (b, c2, semi, semi)):
            got = plane_metrics(x, y, pix_fmt=fx, pix_fmt_b=fy, H=H, W=W)
            assert all(_same(g, w) for g, w in zip(got, want)), (fx, fy, H, W)


def test_p010le_low_bits_are_ignored():
    rng = np.random.default_rng(9)
    for H, W in ((37, 53), (64, 96)):  # the second: the 16-byte loads of the histogram kernel
        a, b = Y.random_payload("p010le", 2, H, W, seed=1), Y.random_payload("p010le", 2, H, W, seed=2)  # low six bits random
        clean_a, clean_b = a.copy(), b.copy()
        clean_a[:, 0::2] &= 0xC0
        clean_b[:, 0::2] &= 0xC0
        assert not np.array_equal(a, clean_a)
        dirty_b = clean_b.copy()
        dirty_b[:, 0::2] |= rng.integers(0, 64, dirty_b[:, 0::2].shape).astype(np.uint8)
        for ssim in (True, False):
            want = plane_metrics(clean_a, clean_b, pix_fmt="p010le", H=H, W=W, ssim=ssim)
            for x, y in ((a, b), (a, dirty_b), (clean_a, b)):
                got = plane_metrics(x, y, pix_fmt="p010le", H=H, W=W, ssim=ssim)
                assert all(_same(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("fmt", ["nv12", "p010le"])
def test_batches_are_bit_equal_to_single_frames_and_repeatable(fmt):
    H, W = 75, 107
    top = (1 << Y.depth_of(fmt)) - 1
    rng = np.random.default_rng(5)
    ya, ua, va = Y.split_planes(Y.random_payload(fmt, 16, H, W, seed=7), fmt, H, W)
    near = lambda p: np.clip(p + rng.integers(-6, 7, p.shape), 0, top)  # noqa: E731
    a = Y.join_planes(ya, ua, va, fmt)
    b = Y.join_planes(near(ya), near(ua), near(va), fmt)
    b[3:] = Y.random_payload(fmt, 13, H, W, seed=8)  # every pair different
    single = [plane_metrics(a[i], b[i], pix_fmt=fmt, H=H, W=W)[0] for i in range(16)]
    assert len({np.array(m.ssim).tobytes() for m in single}) == 16
    for n in (1, 3, 16):
        got = plane_metrics(a[16 - n:], b[16 - n:], pix_fmt=fmt, H=H, W=W)
        again = plane_metrics(a[16 - n:], b[16 - n:], pix_fmt=fmt, H=H, W=W)
        assert len(got) == n
        for i in range(n):
            assert _same(got[i], single[16 - n + i]), (n, i)
            assert _same(got[i], again[i]), (n, i)
    more = plane_metrics(np.concatenate([a, a[:5]]), np.concatenate([b, b[:5]]), pix_fmt=fmt, H=H, W=W)  # 21 frames: two chunks
    assert len(more) == 21 and all(_same(more[i], single[i % 16]) for i in range(21))


def test_bad_arguments_launch_nothing():
    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import PLANE_RECORD_BYTES
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 16, 16
    size = Y.frame_size("p010le", H, W)  # the largest payload asked for below, and a spare sample for the odd address
    d_a, d_b = ctx.upload(np.zeros(size + 2, np.uint8)), ctx.upload(np.full(size + 2, 64, np.uint8))
    d_out = ctx.upload(np.full(PLANE_RECORD_BYTES, 0xAB, np.uint8))
    fn = _lib.lib.avx_plane_metrics
    NV12, P010, Y422, Y444, GRAY = (_lib.AVX_PIX_FMTS[k] for k in ("nv12", "p010le", "yuv422p", "yuv444p", "gray"))
    try:
        for args in ((NV12, None, NV12, d_b.ptr, 1, H, W, d_out.ptr), (NV12, d_a.ptr, NV12, None, 1, H, W, d_out.ptr),
                     (NV12, d_a.ptr, NV12, d_b.ptr, 1, H, W, None), (NV12, d_a.ptr, NV12, d_b.ptr, 0, H, W, d_out.ptr),
                     (NV12, d_a.ptr, NV12, d_b.ptr, 17, H, W, d_out.ptr), (-1, d_a.ptr, NV12, d_b.ptr, 1, H, W, d_out.ptr),
                     (NV12, d_a.ptr, 9, d_b.ptr, 1, H, W, d_out.ptr), (NV12, d_a.ptr, NV12, d_b.ptr, 1, 0, W, d_out.ptr),
                     (NV12, d_a.ptr, NV12, d_b.ptr, 1, H, -3, d_out.ptr), (NV12, d_a.ptr, NV12, d_b.ptr, 1, 1 << 16, 1 << 16, d_out.ptr),
                     (NV12, d_a.ptr, P010, d_b.ptr, 1, H, W, d_out.ptr), (NV12, d_a.ptr, Y422, d_b.ptr, 1, H, W, d_out.ptr),
                     (GRAY, d_a.ptr, Y444, d_b.ptr, 1, H, W, d_out.ptr), (P010, d_a.ptr + 1, P010, d_b.ptr, 1, H, W, d_out.ptr),
                     (P010, d_a.ptr, P010, d_b.ptr + 1, 1, H, W, d_out.ptr)):
            fa, pa, fb, pb, n, h, w, po = args
            rc = fn(ctx._h, fa, pa, fb, pb, n, h, w, 1, po, ctx.stream)
            assert rc == _lib.AVX_ERR_INVALID, args
            assert _lib.lib.avx_last_error(ctx._h).decode().startswith("avx_plane_metrics:"), args
        ctx.sync()
        assert (ctx.download(d_out, (PLANE_RECORD_BYTES,), np.uint8) == 0xAB).all()  # nothing was launched, nothing cleared
        assert fn(ctx._h, P010, d_a.ptr, P010, d_b.ptr, 1, H, W, 1, d_out.ptr, ctx.stream) == 0  # and the good call still works
        rec = np.frombuffer(ctx.download(d_out, (PLANE_RECORD_BYTES,), np.uint8).tobytes(), np.uint32, count=3072).reshape(3, 1024)
        assert [int(v) for v in rec[:, 257]] == [H * W, 64, 64]  # 0x4040 >> 6 = 257 against 0
    finally:
        for d in (d_a, d_b, d_out):
            d.free()


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from animal_vision_amd.renderers import VideoRenderer

    d = tmp_path_factory.mktemp("plane_clips")
    H, W, N = 48, 64, 12
    rng = np.random.default_rng(11)
    base = np.kron(rng.integers(0, 256, (N, 12, 16, 3), dtype=np.uint8), np.ones((1, 4, 4, 1), np.uint8))
    frames = np.clip(base.astype(np.int16) + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8)
    for name, part in (("twelve.y4m", frames), ("nine.y4m", frames[:9])):
        vr = VideoRenderer(read_path=None, write_path=str(d / name))
        vr.open()
        for f in part:
            vr.render(f)
        vr.close()
    vr = VideoRenderer(read_path=str(d / "twelve.y4m"))
    vr.open()
    i420 = np.stack([vr.get_yuv().copy() for _ in range(N)])
    assert vr.get_yuv() is None
    vr.close()
    y, u, v = Y.split_planes(i420, "yuv420p", H, W)
    Y.join_planes(y, u, v, "nv12").tofile(d / "same.nv12")
    y3 = y.copy()
    y3[5, 7, 9] += 3 if y3[5, 7, 9] < 200 else -3
    Y.join_planes(y3, u, v, "nv12").tofile(d / "luma3.nv12")
    p = Y.random_payload("p010le", N, H, W, seed=12)
    p[:, 0::2] &= 0xC0
    py, pu, pv = Y.split_planes(p, "p010le", H, W)
    py1 = py.copy()
    py1[4, 20, 30] += 1 if py1[4, 20, 30] < 1023 else -1
    p.tofile(d / "a.p010")
    Y.join_planes(py1, pu, pv, "p010le").tofile(d / "b.p010")
    Y.join_planes(py, pu, pv, "yuv420p10le").tofile(d / "a.yuv420p10")
    return d


def _compare(capsys, argv):
    from animal_vision_amd import compare

    status = compare.main([str(v) for v in argv])
    cap = capsys.readouterr()
    return status, cap.out, cap.err


def test_command_y4m_against_itself(clips, capsys):
    status, out, err = _compare(capsys, [clips / "twelve.y4m", clips / "twelve.y4m", "--planes", "yuv", "--batch", "5"])
    lines = out.splitlines()
    assert status == 0 and len(lines) == 13 and lines[0] == "frame,psnr_y,psnr_u,psnr_v,psnr,ssim_y,ssim_u,ssim_v,ssim,max_abs,beyond1"
    for i, line in enumerate(lines[1:]):
        assert line == f"{i},inf,inf,inf,inf,1.000000,1.000000,1.000000,1.000000,0,0"
    assert "compare: 12 frames, PSNR-Y inf dB, PSNR inf dB (8-bit)" in err


def test_command_y4m_against_raw_nv12(clips, capsys):
    raw = ["--pix-fmt", "nv12", "--size", "64x48", "--planes", "yuv"]
    status, out, err = _compare(capsys, [clips / "twelve.y4m", clips / "same.nv12"] + raw)
    assert status == 0 and all(line.split(",")[1:5] == ["inf"] * 4 for line in out.splitlines()[1:])
    status, out, err = _compare(capsys, [clips / "twelve.y4m", clips / "luma3.nv12", "--matrix", "bt709", "--range", "full"] + raw)
    lines = [line.split(",") for line in out.splitlines()[1:]]
    assert status == 0 and len(lines) == 12
    want_y = 10 * math.log10(255.0 ** 2 * 48 * 64 / 9)
    for i, f in enumerate(lines):
        if i == 5:
            assert f[1] == f"{want_y:.6f}" and f[2:4] == ["inf", "inf"] and f[9] == "3" and float(f[10]) == pytest.approx(1 / 4608)
            assert f[4] == f"{10 * math.log10(255.0 ** 2 * 4608 / 9):.6f}" and f[6:8] == ["1.000000", "1.000000"] and float(f[5]) < 1.0
        else:
            assert f[1:] == ["inf"] * 4 + ["1.000000"] * 4 + ["0", "0"]
    assert "largest difference 3" in err and "(8-bit)" in err
    status, out, err = _compare(capsys, [clips / "luma3.nv12", clips / "twelve.y4m", "--max-abs", "2", "--no-ssim"] + raw)
    assert status == 1 and "compare: frame 5:" in err and out.splitlines()[6].split(",")[5:9] == ["nan"] * 4


def test_command_p010le_one_code_apart(clips, capsys):
    raw = ["--pix-fmt", "p010le", "--size", "64x48"]
    status, out, err = _compare(capsys, [clips / "a.p010", clips / "b.p010", "--max-abs", "1", "--max-beyond1", "0", "--planes", "yuv"] + raw)
    lines = [line.split(",") for line in out.splitlines()[1:]]
    assert status == 0 and "(10-bit)" in err and "largest difference 1" in err
    assert lines[4][1] == f"{10 * math.log10(1023.0 ** 2 * 3072):.6f}" and lines[4][9:] == ["1", "0"] and lines[3][9] == "0"
    status, out, err = _compare(capsys, [clips / "a.p010", clips / "b.p010", "--max-abs", "0", "--planes", "yuv"] + raw)
    assert status == 1 and "compare: frame 4: largest difference 1 is above --max-abs 0" in err
    # through RGB the pair mostly vanishes: a quarter of an 8-bit code moves a rounded RGB sample by one code at the most, and
    # nothing in the eleven frames that are equal
    status, out, err = _compare(capsys, [clips / "a.p010", clips / "b.p010", "--max-abs", "1"] + raw)
    assert status == 0 and all(line.split(",")[9] == "0" for i, line in enumerate(out.splitlines()[1:]) if i != 4)
    # two layouts of one clip, named by the library call (the command line names one --pix-fmt for both raw inputs)
    n = Y.frame_size("p010le", 48, 64)
    a = np.fromfile(clips / "a.p010", np.uint8).reshape(-1, n)
    b = np.fromfile(clips / "a.yuv420p10", np.uint8).reshape(-1, n)
    assert all(m.max_abs == 0 and m.ssim == (1.0, 1.0, 1.0) for m in plane_metrics(a, b, pix_fmt="p010le", pix_fmt_b="yuv420p10le", H=48, W=64))


def test_command_planes_rgb_is_the_command_without_the_option(clips, capsys):
    for argv in ([clips / "same.nv12", clips / "luma3.nv12", "--pix-fmt", "nv12", "--size", "64x48"],
                 [clips / "twelve.y4m", clips / "nine.y4m", "--batch", "4"],
                 [clips / "a.p010", clips / "b.p010", "--pix-fmt", "p010le", "--size", "64x48", "--no-ssim"]):
        s0, out0, err0 = _compare(capsys, argv)
        s1, out1, err1 = _compare(capsys, argv + ["--planes", "rgb"])
        assert (s0, out0) == (s1, out1) and out0.startswith("frame,psnr_r,")
        assert err0.split(" beyond +-1 code ")[0] == err1.split(" beyond +-1 code ")[0]  # all but the fps figure


def test_command_lengths(clips, capsys):
    status, out, err = _compare(capsys, [clips / "nine.y4m", clips / "twelve.y4m", "--planes", "yuv"])
    assert status == 2 and len(out.splitlines()) == 10 and "B has more frames" in err
    status, out, err = _compare(capsys, [clips / "twelve.y4m", clips / "nine.y4m", "--planes", "yuv", "--shortest", "--batch", "3"])
    assert status == 0 and len(out.splitlines()) == 10 and "more frames" not in err
    (clips / "small.nv12").write_bytes(bytes(40 * 64 * 3 // 2))
    with pytest.raises(SystemExit, match="frame sizes differ"):
        _compare(capsys, [clips / "twelve.y4m", clips / "small.nv12", "--planes", "yuv", "--pix-fmt", "nv12", "--size", "64x40"])
