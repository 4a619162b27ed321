"""No GPU: which C entry point a decode or an encode reaches, and with which arguments (yuv.Decode, yuv.Encode) -- each row of the
dispatch table, the ten public functions against the values they construct, the pipeline's and the renderer's settings against
the values one would write by hand, and the checks that come before the device.

yuv.lib is replaced by a recorder: the six decode and two encode entry points are recorded (name, arguments) and answer 0,
everything else (frame sizes, coefficient tables) goes to the real library.  Contexts and buffers are fakes."""
import numpy as np
import pytest

import _rawyuv_ref as R
import _yuv_ref as Y

H, W, N = 18, 22, 2
HANDLE, STREAM = 0xC0DE, 0x57
DECODES = ("avx_i420_to_rgb_u8", "avx_yuv_to_rgb_u8", "avx_yuv_hdr_to_rgb_u8", "avx_yuv_to_rgb_scaled_u8", "avx_yuv_hdr_to_rgb_scaled_u8")
ENCODES = ("avx_rgb_to_i420_u8", "avx_rgb_to_yuv_u8")
# include/avx.h: enum avx_pix_fmt, AVX_YUV_BT601 / BT709, full_range, enum avx_transfer, enum avx_tonemap
YUV420P, NV12, P010LE, BT601, BT709, LIMITED, FULL, PQ, HLG, CLIP, MOBIUS = 0, 1, 8, 0, 1, 0, 1, 1, 2, 0, 1


class Recorder:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in DECODES or name in ENCODES:
            return lambda *args: self.calls.append((name,) + args) or 0
        return getattr(self.real, name)


class Buf:
    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes, self.freed = ptr, nbytes, 0

    def free(self):
        self.freed += 1


class Ctx:
    """Hands out buffers at addresses that depend only on the order they are asked for in."""
    _h = HANDLE

    def __init__(self):
        self.bufs = []

    def _s(self, stream):
        return 0 if stream is None else stream

    def _check(self, rc):
        assert rc == 0

    def malloc(self, nbytes):
        self.bufs.append(Buf(0x1000 * (len(self.bufs) + 1), int(nbytes)))
        return self.bufs[-1]

    def upload(self, a):
        return self.malloc(a.nbytes)

    def download(self, buf, shape, dtype):
        assert buf.nbytes >= int(np.prod(shape))
        return np.zeros(shape, dtype)

    def pinned(self, shape, dtype):  # what FramePipeline asks of a context besides
        return self.malloc(int(np.prod(shape)))

    def stream_create(self):
        return STREAM

    def stream_destroy(self, s):
        pass

    def sync(self, s):
        pass


class NoCtx:
    def __getattr__(self, name):
        raise AssertionError("the device was asked for")


@pytest.fixture
def rec(monkeypatch):
    from animal_vision_amd import yuv

    r = Recorder(yuv.lib)
    monkeypatch.setattr(yuv, "lib", r)
    return r


def _bufs(yuv_bytes, rgb_hw=(H, W)):
    return Buf(0xA000, N * yuv_bytes), Buf(0xB000, N * rgb_hw[0] * rgb_hw[1] * 3)


HDR = dict(transfer="hlg", tonemap="clip", peak_nits=4000.0, sdr_white=100.0)
HDR_CODES = (HLG, CLIP, 4000.0, 100.0)
# (Decode settings, the payload's format in the reference's terms, entry point, the arguments between the pointers and the stream)
DECODE_ROWS = [
    (dict(matrix="bt709", range="full"), "yuv420p", "avx_i420_to_rgb_u8", None, (N, H, W, BT709, FULL)),
    (dict(matrix="bt709", scale=(9, 7)), "yuv420p", "avx_yuv_to_rgb_scaled_u8", YUV420P, (N, H, W, 7, 9, BT709, LIMITED)),
    (dict(pix_fmt="nv12", range="full"), "nv12", "avx_yuv_to_rgb_u8", NV12, (N, H, W, BT601, FULL)),
    (dict(pix_fmt="nv12", matrix="bt709", scale=(9, 7)), "nv12", "avx_yuv_to_rgb_scaled_u8", NV12, (N, H, W, 7, 9, BT709, LIMITED)),
    (dict(pix_fmt="p010le", range="full", **HDR), "p010le", "avx_yuv_hdr_to_rgb_u8", P010LE, (N, H, W, FULL) + HDR_CODES),
    (dict(pix_fmt="p010le", scale=(9, 7), **HDR), "p010le", "avx_yuv_hdr_to_rgb_scaled_u8", P010LE, (N, H, W, 7, 9, LIMITED) + HDR_CODES),
    # a scale equal to the source size still takes the scaled entry point
    (dict(scale=(W, H)), "yuv420p", "avx_yuv_to_rgb_scaled_u8", YUV420P, (N, H, W, H, W, BT601, LIMITED)),
    (dict(pix_fmt="nv12", scale=(W, H)), "nv12", "avx_yuv_to_rgb_scaled_u8", NV12, (N, H, W, H, W, BT601, LIMITED)),
    (dict(pix_fmt="p010le", scale=(W, H), transfer="pq"), "p010le", "avx_yuv_hdr_to_rgb_scaled_u8", P010LE,
     (N, H, W, H, W, LIMITED, PQ, MOBIUS, 1000.0, 203.0)),
]


@pytest.mark.parametrize("settings,fmt,entry,code,ints", DECODE_ROWS)
def test_each_decode_row_makes_one_call_to_its_entry_point(rec, settings, fmt, entry, code, ints):
    from animal_vision_amd.yuv import Decode

    dec = Decode(**settings)
    out_hw = (settings["scale"][1], settings["scale"][0]) if "scale" in settings else (H, W)
    assert dec.frame_bytes(H, W) == R.frame_size(fmt, H, W) and dec.out_hw(H, W) == out_hw
    d_yuv, d_rgb = _bufs(R.frame_size(fmt, H, W), out_hw)  # exactly as large as needed
    dec.launch(Ctx(), d_yuv, d_rgb, N, H, W, stream=STREAM)
    lead = (HANDLE,) if code is None else (HANDLE, code)
    assert rec.calls == [(entry,) + lead + (0xA000, 0xB000) + ints + (STREAM,)]
    rec.calls.clear()
    dec.launch(Ctx(), d_yuv, d_rgb, N, H, W)  # no stream: the context's own
    assert len(rec.calls) == 1 and rec.calls[0][0] == entry and rec.calls[0][-1] == 0


@pytest.mark.parametrize("settings,fmt,entry,code", [(dict(matrix="bt709", range="full"), "yuv420p", "avx_rgb_to_i420_u8", None),
                                                     (dict(pix_fmt="p010le", matrix="bt709", range="full"), "p010le", "avx_rgb_to_yuv_u8", P010LE)])
def test_each_encode_row_makes_one_call_to_its_entry_point(rec, settings, fmt, entry, code):
    from animal_vision_amd.yuv import Encode

    enc = Encode(**settings)
    assert enc.frame_bytes(H, W) == R.frame_size(fmt, H, W)
    d_yuv, d_rgb = _bufs(R.frame_size(fmt, H, W))
    enc.launch(Ctx(), d_rgb, d_yuv, N, H, W, stream=STREAM)
    lead = (HANDLE,) if code is None else (HANDLE, code)
    assert rec.calls == [(entry,) + lead + (0xB000, 0xA000, N, H, W, BT709, FULL, STREAM)]


def test_each_legacy_function_records_the_call_of_the_value_it_constructs(rec):
    from animal_vision_amd import yuv
    from animal_vision_amd.yuv import Decode, Encode

    mr = dict(matrix="bt709", range="full")
    hdr = dict(range="full", **HDR)
    big = Buf(0xA000, 1 << 20), Buf(0xB000, 1 << 20)
    device = [  # (the legacy call, the value's launch): both get (ctx, source, destination)
        (lambda c, a, b: yuv.i420_to_rgb_device(c, a, b, N, H, W, stream=STREAM, **mr), Decode(None, **mr)),
        (lambda c, a, b: yuv.rgb_to_i420_device(c, a, b, N, H, W, stream=STREAM, **mr), Encode(None, **mr)),
        (lambda c, a, b: yuv.yuv_to_rgb_device(c, "nv12", a, b, N, H, W, stream=STREAM, **mr), Decode("nv12", **mr)),
        (lambda c, a, b: yuv.rgb_to_yuv_device(c, "nv12", a, b, N, H, W, stream=STREAM, **mr), Encode("nv12", **mr)),
        (lambda c, a, b: yuv.yuv_hdr_to_rgb_device(c, "p010le", a, b, N, H, W, stream=STREAM, **hdr), Decode("p010le", **hdr)),
        (lambda c, a, b: yuv.yuv_to_rgb_scaled_device(c, "nv12", a, b, N, H, W, 7, 9, stream=STREAM, **mr), Decode("nv12", scale=(9, 7), **mr)),
        (lambda c, a, b: yuv.yuv_hdr_to_rgb_scaled_device(c, "p010le", a, b, N, H, W, 7, 9, stream=STREAM, **hdr),
         Decode("p010le", scale=(9, 7), **hdr)),
    ]
    for legacy, value in device:
        legacy(Ctx(), *big)
        value.launch(Ctx(), *big, N, H, W, stream=STREAM)
        assert len(rec.calls) == 2 and rec.calls[0] == rec.calls[1], value
        rec.calls.clear()

    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)

    def pay(fmt):
        return rng.integers(0, 256, (N, R.frame_size(fmt, H, W)), dtype=np.uint8)

    i420, nv12, p010 = pay("yuv420p"), pay("nv12"), pay("p010le")
    arrays = [  # (the legacy call, the value's arrays, the result's shape): both get the context
        (lambda c: yuv.i420_to_rgb(i420, H, W, ctx=c, **mr), lambda c: Decode(None, **mr).arrays(i420, H, W, c), (N, H, W, 3)),
        (lambda c: yuv.rgb_to_i420(rgb, ctx=c, **mr), lambda c: Encode(None, **mr).arrays(rgb, c), (N, Y.i420_size(H, W))),
        (lambda c: yuv.yuv_to_rgb(nv12, H, W, pix_fmt="nv12", ctx=c, **mr), lambda c: Decode("nv12", **mr).arrays(nv12, H, W, c), (N, H, W, 3)),
        (lambda c: yuv.rgb_to_yuv(rgb, pix_fmt="nv12", ctx=c, **mr), lambda c: Encode("nv12", **mr).arrays(rgb, c), (N, R.frame_size("nv12", H, W))),
        (lambda c: yuv.yuv_hdr_to_rgb(p010, H, W, pix_fmt="p010le", ctx=c, **hdr), lambda c: Decode("p010le", **hdr).arrays(p010, H, W, c), (N, H, W, 3)),
        (lambda c: yuv.yuv_to_rgb_scaled(nv12, H, W, 7, 9, pix_fmt="nv12", ctx=c, **mr),
         lambda c: Decode("nv12", scale=(9, 7), **mr).arrays(nv12, H, W, c), (N, 7, 9, 3)),
        (lambda c: yuv.yuv_hdr_to_rgb_scaled(p010, H, W, 7, 9, pix_fmt="p010le", ctx=c, **hdr),
         lambda c: Decode("p010le", scale=(9, 7), **hdr).arrays(p010, H, W, c), (N, 7, 9, 3)),
    ]
    for legacy, value, shape in arrays:
        ctxs = Ctx(), Ctx()
        assert legacy(ctxs[0]).shape == value(ctxs[1]).shape == shape
        assert len(rec.calls) == 2 and rec.calls[0] == rec.calls[1], shape
        assert rec.calls[0][-1] == 0 and rec.calls[0][1] == HANDLE
        for c in ctxs:  # the upload and the result: both freed, once
            assert [b.freed for b in c.bufs] == [1, 1]
        rec.calls.clear()
    # one frame in, one frame out
    assert yuv.yuv_to_rgb(nv12[0], H, W, pix_fmt="nv12", ctx=Ctx()).shape == (H, W, 3)
    assert Encode("nv12").arrays(rgb[0], Ctx()).shape == (R.frame_size("nv12", H, W),)
    # the names the legacy functions require stay required: None is not read as I420 or as SDR
    for call in (lambda: yuv.yuv_to_rgb_device(NoCtx(), None, *big, N, H, W), lambda: yuv.rgb_to_yuv_device(NoCtx(), None, *big, N, H, W),
                 lambda: yuv.yuv_to_rgb_scaled_device(NoCtx(), None, *big, N, H, W, 7, 9),
                 lambda: yuv.yuv_hdr_to_rgb_device(NoCtx(), "p010le", *big, N, H, W, transfer=None),
                 lambda: yuv.yuv_hdr_to_rgb_scaled_device(NoCtx(), "p010le", *big, N, H, W, 7, 9, transfer=None)):
        with pytest.raises(ValueError):
            call()


def test_construction_checks_what_needs_no_size_and_no_device():
    from animal_vision_amd.yuv import Decode, Encode

    for bad, word in ((dict(matrix="bt2020"), "matrix must be one of"), (dict(range="tv"), "range must be one of"),
                      (dict(pix_fmt="nv21"), "pix_fmt must be one of"), (dict(transfer="pq"), "10-bit formats"),
                      (dict(pix_fmt="nv12", transfer="pq"), "10-bit formats"), (dict(pix_fmt="p010le", transfer="srgb"), "transfer must be one of"),
                      (dict(pix_fmt="p010le", transfer="pq", tonemap="hable"), "tonemap must be one of"),
                      (dict(pix_fmt="p010le", transfer="pq", peak_nits=100.0), "peak_nits > sdr_white"),
                      (dict(scale=5), r"scale is \(Wd, Hd\)"), (dict(scale=(5,)), r"scale is \(Wd, Hd\)"), (dict(scale=(5, 3, 1)), r"scale is \(Wd, Hd\)")):
        with pytest.raises(ValueError, match=word):
            Decode(**bad)
    for bad, word in ((dict(matrix="bt2020"), "matrix must be one of"), (dict(range="tv"), "range must be one of"),
                      (dict(pix_fmt="nv21"), "pix_fmt must be one of")):
        with pytest.raises(ValueError, match=word):
            Encode(**bad)
    assert Decode(scale=[9, 7]) == Decode(scale=(9, 7)) and hash(Decode(scale=[9, 7])) == hash(Decode(scale=(9, 7)))
    with pytest.raises(AttributeError):  # frozen
        Decode().matrix = "bt709"


def test_checks_precede_the_recorder_and_the_context(rec):
    from animal_vision_amd.yuv import Decode, Encode

    fsz = R.frame_size("nv12", H, W)
    ok_yuv, ok_rgb, ok_small = Buf(0, N * fsz), Buf(0, N * H * W * 3), Buf(0, N * 7 * 9 * 3)
    plain, scaled = Decode("nv12"), Decode("nv12", scale=(9, 7))
    for call, word in (
            (lambda: plain.launch(NoCtx(), Buf(0, N * fsz - 1), ok_rgb, N, H, W), "need"),            # an undersized source
            (lambda: plain.launch(NoCtx(), ok_yuv, Buf(0, N * H * W * 3 - 1), N, H, W), "need"),       # an undersized destination
            (lambda: scaled.launch(NoCtx(), Buf(0, N * fsz - 1), ok_small, N, H, W), "need"),
            (lambda: scaled.launch(NoCtx(), ok_yuv, Buf(0, N * 7 * 9 * 3 - 1), N, H, W), "need"),
            (lambda: Decode().launch(NoCtx(), Buf(0, N * Y.i420_size(H, W) - 1), ok_rgb, N, H, W), "need"),
            (lambda: plain.launch(NoCtx(), ok_yuv, ok_rgb, 0, H, W), "bad shape"),
            (lambda: scaled.launch(NoCtx(), ok_yuv, ok_rgb, 0, H, W), "bad shape"),
            (lambda: Decode("nv12", scale=(W + 1, H)).launch(NoCtx(), ok_yuv, ok_rgb, N, H, W), "enlarges"),
            (lambda: Decode(scale=(W, H + 1)).launch(NoCtx(), ok_yuv, ok_rgb, N, H, W), "enlarges"),
            (lambda: Decode("p010le", transfer="pq", scale=(W, H + 1)).launch(NoCtx(), Buf(0, 1 << 20), ok_rgb, N, H, W), "enlarges"),
            (lambda: Decode("nv12", scale=(W + 1, H)).out_hw(H, W), "enlarges"),
            (lambda: Encode("nv12").launch(NoCtx(), Buf(0, N * H * W * 3 - 1), ok_yuv, N, H, W), "need"),
            (lambda: Encode("nv12").launch(NoCtx(), ok_rgb, Buf(0, N * fsz - 1), N, H, W), "need"),
            (lambda: Encode().launch(NoCtx(), ok_rgb, Buf(0, N * Y.i420_size(H, W) - 1), N, H, W), "need"),
            (lambda: Encode().launch(NoCtx(), ok_rgb, ok_yuv, 0, H, W), "bad shape")):
        with pytest.raises(ValueError, match=word):
            call()
    assert rec.calls == []
    with pytest.raises(AssertionError, match="the device was asked for"):  # good arguments do reach the context
        scaled.launch(NoCtx(), ok_yuv, ok_small, N, H, W)
    # arrays: a payload that is not uint8 is a TypeError, one of the wrong size a ValueError, both before a context is asked for
    with pytest.raises(TypeError):
        plain.arrays(np.zeros(fsz // 2, np.uint16), H, W, NoCtx())
    with pytest.raises(ValueError):
        plain.arrays(np.zeros(fsz - 1, np.uint8), H, W, NoCtx())
    with pytest.raises(ValueError):
        Encode().arrays(np.zeros((H, W, 3), np.float32), NoCtx())
    assert rec.calls == []


class Op:  # never run: the pipelines below are built and closed
    ctx = None


def _pipeline(**kw):
    from animal_vision_amd.pipeline import FramePipeline

    return FramePipeline(Op(), H, W, ctx=Ctx(), depth=1, **kw)


def test_pipeline_keywords_and_the_pair_given_directly_agree():
    from animal_vision_amd.pipeline import FramePipeline
    from animal_vision_amd.yuv import Decode, Encode

    cases = [
        (dict(io_format="i420", matrix="bt709", yuv_range="full"), Decode(None, "bt709", "full"), Encode(None, "bt709", "full")),
        (dict(io_format="i420", scale=(9, 7)), Decode(scale=(9, 7)), Encode()),
        (dict(io_format="yuv", pix_fmt="nv12", out_matrix="bt709"), Decode("nv12"), Encode("nv12", "bt709")),
        (dict(io_format="yuv", pix_fmt="nv12", matrix="bt709", scale=(9, 7)), Decode("nv12", "bt709", scale=(9, 7)), Encode("nv12", "bt709")),
        (dict(io_format="yuv", pix_fmt="p010le", yuv_range="full", **HDR), Decode("p010le", range="full", **HDR), Encode("p010le", "bt709", "full")),
        (dict(io_format="yuv", pix_fmt="p010le", transfer="pq", out_matrix="bt601", scale=(9, 7)), Decode("p010le", transfer="pq", scale=(9, 7)),
         Encode("p010le", "bt601")),
    ]
    for kw, decode, encode in cases:
        a, b = _pipeline(**kw), _pipeline(decode=decode, encode=encode)
        assert a.decode == b.decode == decode and a.encode == b.encode == encode, kw
        for name in ("io_format", "pix_fmt", "matrix", "yuv_range", "transfer", "tonemap", "peak_nits", "sdr_white", "out_matrix", "scale",
                     "op_H", "op_W", "out_H", "out_W"):
            assert getattr(a, name) == getattr(b, name), (kw, name)
        assert a.out_matrix == encode.matrix and a.scale == kw.get("scale") and (a.op_H, a.op_W) == ((7, 9) if "scale" in kw else (H, W))
        for p in (a, b):  # the slot's payload buffers are sized by the pair
            s = p.slots[0]
            assert (s.d_yuv_in.nbytes, s.d_yuv_out.nbytes, s.d_full) == (decode.frame_bytes(H, W), encode.frame_bytes(p.out_H, p.out_W), None)
            p.close()
    for kw in (dict(io_format="yuv"), dict(pix_fmt="nv12"), dict(matrix="bt709"), dict(yuv_range="full"), dict(transfer="pq"), dict(tonemap="clip"),
               dict(peak_nits=4000.0), dict(sdr_white=100.0), dict(out_matrix="bt709"), dict(scale=(9, 7))):
        with pytest.raises(ValueError, match=next(iter(kw))):  # the pair and a format keyword: refused, the keyword named
            FramePipeline(Op(), H, W, ctx=NoCtx(), decode=Decode(), encode=Encode(), **kw)
    for kw in (dict(decode=Decode()), dict(encode=Encode())):
        with pytest.raises(ValueError, match="go together"):
            FramePipeline(Op(), H, W, ctx=NoCtx(), **kw)


def test_renderer_settings_equal_the_values_written_by_hand(tmp_path):
    from animal_vision_amd.renderers import VideoRenderer
    from animal_vision_amd.yuv import Decode, Encode

    raw8, raw10, y4m = str(tmp_path / "a.yuv"), str(tmp_path / "b.yuv"), str(tmp_path / "c.y4m")
    R.random_payload("nv12", 1, H, W, 1).tofile(raw8)
    R.random_payload("p010le", 1, H, W, 1).tofile(raw10)
    frame = np.zeros(Y.i420_size(H, W), np.uint8)
    open(y4m, "wb").write(Y.y4m_bytes([frame], H, W, header="F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL"))
    size = (W, H)
    cases = [
        # raw SDR, payloads in and out; without a sink the payloads leave in the source's format
        (dict(read_path=raw8, write_path=str(tmp_path / "o.yuv"), pix_fmt="nv12", size=size, matrix="bt709", range="full"),
         Decode("nv12", "bt709", "full"), Encode("nv12", "bt709", "full")),
        (dict(read_path=raw8, pix_fmt="nv12", size=size), Decode("nv12"), Encode("nv12")),
        (dict(read_path=raw8, write_path=str(tmp_path / "o.y4m"), pix_fmt="nv12", size=size, out_matrix="bt709"), Decode("nv12"), Encode(None, "bt709")),
        (dict(read_path=raw8, write_path=str(tmp_path / "p.yuv"), pix_fmt="nv12", size=size, write_pix_fmt="p010le"), Decode("nv12"), Encode("p010le")),
        # raw HDR: bt709 on the way out exactly when a transfer is set and no out_matrix is named
        (dict(read_path=raw10, write_path=str(tmp_path / "q.yuv"), pix_fmt="p010le", size=size, **HDR), Decode("p010le", **HDR), Encode("p010le", "bt709")),
        (dict(read_path=raw10, write_path=str(tmp_path / "r.yuv"), pix_fmt="p010le", size=size, out_matrix="bt601", **HDR),
         Decode("p010le", **HDR), Encode("p010le", "bt601")),
        (dict(read_path=raw10, write_path=str(tmp_path / "s.yuv"), pix_fmt="p010le", size=size), Decode("p010le"), Encode("p010le", "bt601")),
        (dict(read_path=raw10, write_path=str(tmp_path / "t.yuv"), pix_fmt="p010le", size=size, scale=(9, 7), range="full", **HDR),
         Decode("p010le", range="full", scale=(9, 7), **HDR), Encode("p010le", "bt709", "full")),
        # .y4m: I420, the range from the header unless one is named
        (dict(read_path=y4m, write_path=str(tmp_path / "u.y4m"), scale=(9, 7)), Decode(None, "bt601", "full", scale=(9, 7)), Encode(None, "bt601", "full")),
        (dict(read_path=y4m, write_path=str(tmp_path / "v.y4m"), matrix="bt709", range="limited"), Decode(None, "bt709"), Encode(None, "bt709")),
    ]
    for kw, decode, encode in cases:
        vr = VideoRenderer(**kw)
        vr.open()
        try:
            assert vr.decode == decode and vr.encode == encode, kw
            assert (vr.transfer, vr.tonemap, vr.peak_nits, vr.sdr_white, vr.scale) == (decode.transfer, decode.tonemap, decode.peak_nits,
                                                                                     decode.sdr_white, decode.scale)
            assert (vr.matrix, vr.yuv_range, vr.out_matrix) == (decode.matrix, decode.range, encode.matrix)
        finally:
            vr.close()
