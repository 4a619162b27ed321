"""GPU: the dE_ITP kernel (csrc/itp.hip) against the float64 definition of tests/_itp_ref.py, and `deltae --itp` end to
end.  The frames are _itp_ref.CASES': noise, dark, near-copy, ramp and saturated at 1 x 1, 2 x 2, 7 x 13, 16 x 32 and 70 x 530, over
the four 10-bit formats, PQ and HLG, both ranges, and HDR against HDR, HDR against SDR and SDR against SDR.

Accuracy.  BOUND is 8 x the largest deviation of the float32 restatement (_itp_ref.delta32, NumPy's float32 log2 / exp2 on a CPU) from
the definition on these same frames -- 8 x 1.19e-3 = 9.5e-3 --, the margin tests/test_receptor_acuity_gpu.py took for the hardware's
approximate log2 / exp2 / rcp over libm.  Values reach 709, so the bound is 1.3e-5 of the largest.  The device's own deviation is
printed per case and frame; measured on an MI355X the largest is 1.03e-3 (the ramp of yuv420p10le PQ full against yuv422p10le HLG
full at 70 x 530; 9.3e-5 at 1 x 1, 3.2e-4 at 2 x 2, 7.6e-4 at 7 x 13, 9.4e-4 at 16 x 32).

Everything else has no tolerance: exact zeros, the achromatic rule (which is tested on the device's own values alone: on a line the
largest of three distances is the float32 sum of the other two, bit for bit, exactly when T* and P* vanish and the value is the one
subtraction |I*_A - I*_B|), the record and the map against the device's own values, batches, alignment and the two 4:2:0 layouts."""
import numpy as np
import pytest

import _deltae_ref as E
import _itp_ref as I
import _rawyuv_ref as R
from animal_vision_amd import deltae as _deltae_module  # noqa: F401
from test_deltae_gpu import _check_record, _deltae, _rows, _y4m_frames

pytestmark = pytest.mark.gpu

_bound = []


def _BOUND():
    if not _bound:
        _bound.append(8.0 * I.restatement_deviation())
    return _bound[0]


def _side(ref_side, H, W):
    """A side of _itp_ref as metrics takes it."""
    from animal_vision_amd.metrics import HdrFrames

    if ref_side[0] == "sdr":
        return ref_side[1]
    _, payload, fmt, transfer, rng = ref_side
    return HdrFrames(payload, fmt, H, W, transfer, rng)


def _panel(ref_side, H, W, **kw):
    """The uint8 RGB frames a map shows for a side: the side itself, or an HDR side's tone-mapped decode."""
    from animal_vision_amd.yuv import yuv_hdr_to_rgb

    if ref_side[0] == "sdr":
        return ref_side[1]
    _, payload, fmt, transfer, rng = ref_side
    return yuv_hdr_to_rgb(payload, H, W, pix_fmt=fmt, transfer=transfer, range=rng, **kw)


def _neutral(Y, fmt, H, W):
    """(1, frame bytes): luma plane Y (H x W) with neutral chroma."""
    ch, cw = R.plane_shapes(fmt, H, W)
    c = np.full((1, ch, cw), 512)
    return R.join_planes(np.asarray(Y).reshape(1, H, W), c, c, fmt)


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("case", I.CASES, ids=I.case_id)
def test_values_against_the_float64_definition(case):
    from animal_vision_amd.metrics import itp_delta_values

    H, W = case[:2]
    sa, sb, want, _ = I.case_sides(case)
    got = itp_delta_values(_side(sa, H, W), _side(sb, H, W))
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and (got >= 0).all()
    dev = np.abs(got.astype(np.float64) - want).reshape(len(I.KINDS), -1).max(1)
    print(f"itp {I.case_id(case)}: largest |device - definition| " + ", ".join(f"{k} {d:.3e}" for k, d in zip(I.KINDS, dev)) +
          f"; bound {_BOUND():.3e}; largest dE_ITP {want.max():.2f}")
    assert dev.max() <= _BOUND(), (I.case_id(case), float(dev.max()), _BOUND())
    one = itp_delta_values(_side((sa[0], sa[1][1], *sa[2:]), H, W), _side((sb[0], sb[1][1], *sb[2:]), H, W))  # one frame: H x W
    assert one.shape == (H, W) and one.tobytes() == got[1].tobytes()


# ------------------------------------------------------------------------------------------------ exact zeros
@pytest.mark.parametrize("case", [I.CASES[4], I.CASES[7], I.CASES[9], I.CASES[12]], ids=I.case_id)
def test_identical_sides_are_exactly_zero(case):
    from animal_vision_amd.metrics import itp_delta_map, itp_delta_values

    H, W = case[:2]
    sa = I.case_sides(case)[0]
    a = _side(sa, H, W)
    assert not itp_delta_values(a, a).any()
    plain, recs = itp_delta_map(a, a, mode="plain", gain=255.0, threshold=0.0)
    assert not plain.any() and plain.shape == (5, H, W, 3)
    heat, recs_h = itp_delta_map(a, a, mode="heat", gain=255.0, threshold=0.0, layout="side")
    pa = _panel(sa, H, W).astype(np.int64)
    g = (((77 * pa[..., 0] + 150 * pa[..., 1] + 29 * pa[..., 2] + 128) >> 8) >> 2).astype(np.uint8)
    assert np.array_equal(heat[:, :, 2 * W:], np.stack([g, g, g], -1)) and np.array_equal(heat[:, :, :W], pa) and np.array_equal(heat[:, :, W : 2 * W], pa)
    for r in recs + recs_h:
        assert r.hist[0] == H * W and r.hist.sum() == H * W and (r.sum, r.max_de, r.max_x, r.max_y, r.beyond) == (0.0, 0.0, 0, 0, 0)


def test_achromatic_pixels_differ_by_exactly_720_times_the_difference_of_i():
    """Three achromatic sides of different kinds whose I* lie within a factor of two of each other: every float32 subtraction
    I*_X - I*_Y is then exact (Sterbenz), so among the three distances of a pixel the largest is the float32 sum of the other two bit
    for bit -- if and only if every value is the bare |dI*|, with T* = P* = 0 and no root taken."""
    from animal_vision_amd.metrics import itp_delta, itp_delta_values

    H, W = 7, 13
    rng = np.random.default_rng(3)
    s = I.sdr(np.repeat(rng.integers(100, 256, (1, H, W, 1), dtype=np.uint8), 3, axis=3))  # sRGB greys at 203 nits: I from 0.42 to 0.58
    p = I.hdr(_neutral(rng.integers(400, 601, (H, W)), "yuv420p10le", H, W), "yuv420p10le", "pq", "limited")  # I from 0.38 to 0.61
    h = I.hdr(_neutral(rng.integers(500, 801, (H, W)), "yuv444p10le", H, W), "yuv444p10le", "hlg", "full")  # I from 0.44 to 0.60
    d = {}
    for (na, xa), (nb, xb) in (((0, s), (1, p)), ((1, p), (2, h)), ((0, s), (2, h))):
        v = itp_delta_values(_side(xa, H, W), _side(xb, H, W))[0]
        want = I.delta(xa, xb, H, W)[0]
        assert np.abs(v.astype(np.float64) - want).max() <= _BOUND() and v.max() > 10
        assert v.tobytes() == itp_delta_values(_side(xb, H, W), _side(xa, H, W))[0].tobytes()  # |dI*| is symmetric bit for bit
        rec = itp_delta(_side(xa, H, W), _side(xb, H, W))[0]
        assert np.float32(rec.max_de) == v.max()
        d[(na, nb)] = v
    stack = np.sort(np.stack([d[(0, 1)], d[(1, 2)], d[(0, 2)]]), axis=0)
    assert stack.dtype == np.float32 and (stack[0] + stack[1]).tobytes() == stack[2].tobytes()
    # a chroma sample one code off neutral breaks it: the test can fail
    off = R.split_planes(p[1], "yuv420p10le", H, W)
    tinted = I.hdr(R.join_planes(off[0], off[1] + 1, off[2], "yuv420p10le"), "yuv420p10le", "pq", "limited")
    v = itp_delta_values(_side(s, H, W), _side(tinted, H, W))[0]
    broken = np.sort(np.stack([v, d[(1, 2)], itp_delta_values(_side(tinted, H, W), _side(h, H, W))[0]]), axis=0)
    assert (broken[0] + broken[1] != broken[2]).any()


# ------------------------------------------------------------------------------------------------ the record and the map: no tolerance
@pytest.mark.parametrize("case", [I.CASES[3], I.CASES[5], I.CASES[7], I.CASES[11], I.CASES[13]], ids=I.case_id)
def test_record_and_map_follow_the_devices_own_values(case):
    from animal_vision_amd.metrics import itp_delta, itp_delta_map, itp_delta_values

    H, W = case[:2]
    sa, sb, _, _ = I.case_sides(case)
    a, b = _side(sa, H, W), _side(sb, H, W)
    v = itp_delta_values(a, b)
    pa, pb = _panel(sa, H, W), _panel(sb, H, W)
    for mode, layout, G, T in (("heat", "map", None, 1.0), ("heat", "side", 10.0, 1.0), ("plain", "map", 0.3, 1.0), ("plain", "side", 2.5, 0.0),
                               ("heat", "map", 255.0, 0.0), ("heat", "side", 0.37, 2.3)):
        got, recs = itp_delta_map(a, b, mode=mode, gain=G, threshold=T, layout=layout)
        assert got.dtype == np.uint8 and got.shape == (5, H, W * (3 if layout == "side" else 1), 3)
        only = itp_delta(a, b, threshold=T)
        for i, name in enumerate(I.KINDS):
            what = (name, mode, layout, G, T, H, W)
            m = E.de_map(v[i], pa[i], 10.0 if G is None else G, T, mode)
            assert np.array_equal(got[i], E.side(pa[i], pb[i], m) if layout == "side" else m), what
            _check_record(recs[i], v[i], T, what)
            assert only[i] == recs[i], what  # records only (no map) is the same record
    if sa[0] == "hdr":  # the panels follow the tone map that is asked for
        clip, _ = itp_delta_map(a, b, layout="side", tonemap="clip", peak_nits=600.0, sdr_white=100.0)
        pc = _panel(sa, H, W, tonemap="clip", peak_nits=600.0, sdr_white=100.0)
        assert np.array_equal(clip[:, :, :W], pc) and not np.array_equal(pc, pa)


# ------------------------------------------------------------------------------------------------ batches and alignment
def test_a_frame_does_not_depend_on_its_batch_or_on_the_alignment_of_the_buffers():
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, ItpSide, delta_e_records_from_bytes, itp_delta_launch, itp_delta_map, itp_delta_values
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    for case in (I.CASES[8], I.CASES[11]):  # 16 x 32 (16-byte runs where aligned) and 70 x 530, HDR against SDR
        H, W = case[:2]
        sa, sb, _, _ = I.case_sides(case)
        _, payload, fmt, tr, rng = sa
        payload, rgb = payload[:3], sb[1][:3]
        a, b = _side(("hdr", payload, fmt, tr, rng), H, W), rgb
        maps, recs = itp_delta_map(a, b, layout="side")
        vals = itp_delta_values(a, b)
        for i in (0, 2):  # alone, and at places 0 and 2 of a batch of 3
            m1, r1 = itp_delta_map(_side(("hdr", payload[i], fmt, tr, rng), H, W), rgb[i], layout="side")
            assert np.array_equal(m1, maps[i]) and r1 == recs[i]
            assert itp_delta_values(_side(("hdr", payload[i], fmt, tr, rng), H, W), rgb[i]).tobytes() == vals[i].tobytes()
        # the same three frames from buffers that are offset: the payload by 2 bytes, RGB, panel and map by 1
        n, fsz, fb = 3, payload.shape[1], H * W * 3
        panel = _panel(("hdr", payload, fmt, tr, rng), H, W)
        bufs = [ctx.malloc(n * fsz + 32), ctx.malloc(n * fb + 32), ctx.malloc(n * fb + 32), ctx.malloc(3 * n * fb + 32), ctx.malloc(n * DELTA_E_RECORD_BYTES),
                ctx.malloc(n * H * W * 4)]
        try:
            d_y, d_b, d_p, d_o, d_r, d_v = bufs
            for off_y, off_b, off_p, off_o in ((2, 1, 1, 1), (2, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (8, 8, 8, 8), (0, 0, 0, 0)):
                vy, vb, vp, vo = d_y.view(off_y, n * fsz), d_b.view(off_b, n * fb), d_p.view(off_p, n * fb), d_o.view(off_o, 3 * n * fb)
                ctx.upload(payload, vy), ctx.upload(rgb, vb), ctx.upload(panel, vp)
                itp_delta_launch(ctx, ItpSide(vy, fmt, tr, rng, vp), ItpSide(vb), n, H, W, vo, d_r, layout="side", d_float=d_v)
                what = (H, W, off_y, off_b, off_p, off_o)
                assert np.array_equal(ctx.download(vo, (n, H, 3 * W, 3), np.uint8), maps), what
                assert delta_e_records_from_bytes(ctx.download(d_r, (n * DELTA_E_RECORD_BYTES,), np.uint8), n) == recs, what
                assert ctx.download(d_v, (n, H, W), np.float32).tobytes() == vals.tobytes(), what
                # the sides swapped: SDR first
                itp_delta_launch(ctx, ItpSide(vb), ItpSide(vy, fmt, tr, rng, vp), n, H, W, None, d_r, d_float=d_v)
                assert ctx.download(d_v, (n, H, W), np.float32).tobytes() == vals.tobytes(), what
        finally:
            for d in bufs:
                d.free()


# ------------------------------------------------------------------------------------------------ formats
@pytest.mark.parametrize("H,W", [(7, 13), (16, 32)])
def test_yuv420p10le_and_p010le_of_the_same_samples_are_one_side(H, W):
    from animal_vision_amd.metrics import itp_delta, itp_delta_values

    planar = I.hdr_pair("yuv420p10le", H, W, 77)[0]
    semi = R.join_planes(*R.split_planes(planar, "yuv420p10le", H, W), "p010le")
    assert semi.shape == planar.shape and not np.array_equal(semi, planar)
    for tr, rng in (("pq", "limited"), ("hlg", "full")):
        a, b = _side(I.hdr(planar, "yuv420p10le", tr, rng), H, W), _side(I.hdr(semi, "p010le", tr, rng), H, W)
        assert not itp_delta_values(a, b).any() and all(r.max_de == 0.0 and r.hist[0] == H * W for r in itp_delta(a, b))
        third = I.sdr_pair(H, W, 5)[1]
        va, vb = itp_delta_values(a, third), itp_delta_values(b, third)
        assert va.any() and va.tobytes() == vb.tobytes()
        other = _side(I.hdr(I.hdr_pair("yuv422p10le", H, W, 78)[1], "yuv422p10le", "pq", "full"), H, W)
        assert itp_delta_values(other, a).tobytes() == itp_delta_values(other, b).tobytes()


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_launch_nothing():
    import ctypes

    from animal_vision_amd import _lib
    from animal_vision_amd.metrics import DELTA_E_RECORD_BYTES, delta_e_records_from_bytes
    from animal_vision_amd.runtime import get_context

    ctx = get_context()
    H, W = 16, 16
    fb, fsz = H * W * 3, R.frame_size("p010le", H, W)
    d_in = ctx.upload(np.zeros(4 * fb, np.uint8))  # SDR a, HDR b (768 bytes: as many as an RGB frame), b's panel, and room behind them
    d_out = ctx.upload(np.full(3 * fb, 0xAB, np.uint8))
    d_rec = ctx.upload(np.full(DELTA_E_RECORD_BYTES + 8, 0xAB, np.uint8))
    d_val = ctx.upload(np.full(H * W * 4 + 4, 0xAB, np.uint8))
    a, b, pb = d_in.ptr, d_in.ptr + fb, d_in.ptr + 2 * fb
    o, r, v = d_out.ptr, d_rec.ptr, d_val.ptr
    fn = _lib.lib.avx_itp_delta
    P010, NV12, GRAY, PQ, HLG = 8, 1, 4, 1, 2
    nan, inf = float("nan"), float("inf")

    def side(kind=0, data=a, panel=None, fmt=0, full=0, tr=0, size=None):
        return _lib.ItpSide(struct_size=ctypes.sizeof(_lib.ItpSide) if size is None else size, kind=kind, data=data, panel=panel, pix_fmt=fmt, full_range=full,
                            transfer=tr)

    sdr, hdr = side(), side(1, b, pb, P010, 0, PQ)
    good = dict(a=sdr, b=hdr, white=203.0, n=1, H=H, W=W, mode=0, gain=10.0, thr=1.0, layout=0, o=o, r=r, v=v)

    def call(**kw):
        k = dict(good, **kw)
        pa, pb_ = (None if s is None else ctypes.byref(s) for s in (k["a"], k["b"]))
        return fn(ctx._h, pa, pb_, k["white"], k["n"], k["H"], k["W"], k["mode"], k["gain"], k["thr"], k["layout"], k["o"], k["r"], k["v"], ctx.stream)

    try:
        bad = [dict(a=None), dict(b=None), dict(a=side(size=32)), dict(b=side(kind=2)), dict(a=side(kind=-1)), dict(a=side(data=None)),
               dict(b=side(1, None, pb, P010, 0, PQ)), dict(r=None),
               dict(n=0), dict(n=17), dict(n=-1), dict(H=0), dict(W=-3), dict(a=sdr, b=sdr, H=1 << 16, W=1 << 16), dict(H=1 << 16, W=4),
               dict(mode=2), dict(mode=-1), dict(layout=2), dict(layout=-1),
               dict(gain=0.0), dict(gain=-1.0), dict(gain=255.5), dict(gain=nan), dict(gain=inf), dict(thr=-0.5), dict(thr=nan), dict(thr=inf),
               dict(r=r + 4), dict(v=v + 2), dict(o=a), dict(o=b + fsz - 1), dict(o=pb), dict(o=a + 1, layout=1),
               dict(b=side(1, b, pb, NV12, 0, PQ)), dict(b=side(1, b, pb, GRAY, 0, PQ)), dict(b=side(1, b, pb, 9, 0, PQ)), dict(b=side(1, b, pb, -1, 0, PQ)),
               dict(b=side(1, b, pb, P010, 2, PQ)), dict(b=side(1, b, pb, P010, 0, 0)), dict(b=side(1, b, pb, P010, 0, 3)),
               dict(b=side(1, b + 1, pb, P010, 0, HLG)), dict(b=side(1, b, None, P010, 0, PQ)),
               dict(white=0.0), dict(white=-203.0), dict(white=nan), dict(white=inf)]
        for kw in bad:
            assert call(**kw) == _lib.AVX_ERR_INVALID, kw
            assert _lib.lib.avx_last_error(ctx._h).decode().startswith("avx_itp_delta:"), kw
        assert fn(None, ctypes.byref(sdr), ctypes.byref(hdr), 203.0, 1, H, W, 0, 10.0, 1.0, 0, o, r, v, ctx.stream) == _lib.AVX_ERR_INVALID  # a NULL context
        ctx.sync()
        assert (ctx.download(d_out, (3 * fb,), np.uint8) == 0xAB).all() and (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8) == 0xAB).all()
        assert (ctx.download(d_val, (H * W * 4 + 4,), np.uint8) == 0xAB).all() and not ctx.download(d_in, (4 * fb,), np.uint8).any()
        # the good call still works: sRGB white at 203 nits against HDR black; an HDR side needs no panel when there is no map
        ctx.upload(np.full(fb, 255, np.uint8), d_in.view(0, fb))
        ctx.upload(_neutral(np.full((H, W), 64), "p010le", H, W), d_in.view(fb, fsz))  # limited-range black, neutral chroma; its panel stays 0
        assert call(mode=1, gain=0.25, layout=1) == 0
        rec = delta_e_records_from_bytes(ctx.download(d_rec, (DELTA_E_RECORD_BYTES,), np.uint8), 1)[0]
        want = 720.0 * (I.pq_inverse(0.0203) - I.pq_inverse(0.0))
        assert abs(rec.max_de - want) <= _BOUND() and (rec.max_x, rec.max_y, rec.beyond) == (0, 0, H * W) and rec.hist[255] == H * W
        out = ctx.download(d_out, (H, 3 * W, 3), np.uint8)
        assert (out[:, :W] == 255).all() and not out[:, W : 2 * W].any() and (out[:, 2 * W:] == E.pal(int(np.floor(np.float32(0.25) * np.float32(rec.max_de) + np.float32(0.5))))).all()
        assert (ctx.download(d_rec, (DELTA_E_RECORD_BYTES + 8,), np.uint8)[DELTA_E_RECORD_BYTES:] == 0xAB).all()  # nothing behind the record
        assert call(b=side(1, b, None, P010, 0, PQ), o=None, v=None) == 0
        assert delta_e_records_from_bytes(ctx.download(d_rec, (DELTA_E_RECORD_BYTES,), np.uint8), 1)[0] == rec
    finally:
        for d in (d_in, d_out, d_rec, d_val):
            d.free()


# ------------------------------------------------------------------------------------------------ the command
def test_command_on_hdr_files_and_against_an_sdr_rendering(capsys, tmp_path):
    from animal_vision_amd.metrics import HdrFrames, itp_delta, itp_delta_map
    from animal_vision_amd.pairs import num
    from animal_vision_amd.renderers import VideoRenderer
    import _yuv_ref

    H = W = 16
    pa, pb = I.hdr_pair("p010le", H, W, 21)
    a, b = pa[[0, 2]], pb[[0, 2]]  # noise against noise, and a frame against its near copy
    a.tofile(tmp_path / "a.yuv"), b.tofile(tmp_path / "b.yuv")
    hdr = ["--pix-fmt", "p010le", "--size", f"{W}x{H}", "--transfer", "pq"]
    A, B = HdrFrames(a, "p010le", H, W, "pq"), HdrFrames(b, "p010le", H, W, "pq")
    # two HDR files, a .y4m of maps and the CSV
    status, stdout, err = _deltae(capsys, [tmp_path / "a.yuv", tmp_path / "b.yuv", tmp_path / "o.y4m", "--csv", tmp_path / "w.csv", "--itp"] + hdr)
    recs = itp_delta(A, B)
    maps, recs_m = itp_delta_map(A, B)
    assert status == 0 and stdout == "" and recs == recs_m
    assert (tmp_path / "w.csv").read_text() == _rows(recs)
    (Wo, Ho), frames = _y4m_frames(tmp_path / "o.y4m")
    assert (Wo, Ho) == (W, H) and np.array_equal(np.stack(frames), _yuv_ref.encode(maps, "bt709"))
    worst = max(r.max_de for r in recs)
    first = next(i for i, r in enumerate(recs) if r.max_de == worst)
    assert f"deltae: 2 frames, mean dE_ITP (pq, sdr white 203) {num(sum(r.mean for r in recs) / 2)}, largest dE {num(worst)} (frame {first}, " in err
    assert recs[0].max_de > 100 > recs[1].max_de > 0  # noise is far apart, the near copy is not
    # one of them against a .y4m: its own SDR rendering
    sdr = A.decode().arrays(a, H, W)
    vr = VideoRenderer(read_path=None, write_path=str(tmp_path / "sdr.y4m"))
    vr.open()
    for f in sdr:
        vr.render(f)
    vr.close()
    vr = VideoRenderer(read_path=str(tmp_path / "sdr.y4m"))
    vr.open()
    seen = np.stack([vr.get_image() for _ in range(2)])  # what the .y4m decodes to: 4:2:0 is lossy
    vr.close()
    status, stdout, err = _deltae(capsys, [tmp_path / "a.yuv", tmp_path / "sdr.y4m", "--itp", "--sdr-white", "100", "--threshold", "3"] + hdr)
    recs = itp_delta(A, seen, 100.0, threshold=3.0)
    assert status == 0 and stdout == _rows(recs) and "mean dE_ITP (pq, sdr white 100)" in err and "pixels beyond 3" in err
    status, stdout, err = _deltae(capsys, [tmp_path / "sdr.y4m", tmp_path / "a.yuv", tmp_path / "side.npy", "--itp", "--layout", "side", "--tonemap", "clip"] + hdr)
    want, _ = itp_delta_map(seen, A, layout="side", tonemap="clip")
    assert status == 0 and np.array_equal(np.load(tmp_path / "side.npy"), want)
    # SDR against SDR names no transfer
    status, stdout, err = _deltae(capsys, [tmp_path / "sdr.y4m", tmp_path / "sdr.y4m", "--itp"])
    assert status == 0 and "mean dE_ITP (sdr white 203) 0.000000, largest dE 0.000000, 0 pixels beyond 1" in err
    # a limit
    recs = itp_delta(A, B)
    status, stdout, err = _deltae(capsys, [tmp_path / "a.yuv", tmp_path / "b.yuv", "--itp", "--max-de", "100"] + hdr)
    assert status == 1 and f"deltae: frame 0: largest dE {num(recs[0].max_de)}" in err and "--max-de 100" in err
    # without --itp: the output deltae gives today, the tone-mapped frames compared as 8-bit sRGB
    from animal_vision_amd.metrics import delta_e

    status, stdout, err = _deltae(capsys, [tmp_path / "a.yuv", tmp_path / "b.yuv"] + hdr)
    assert status == 0 and stdout == _rows(delta_e(sdr, B.decode().arrays(b, H, W))) and "mean dE " in err and "ITP" not in err
