"""No GPU: the host side of the scaled HDR decode -- the exported symbol and its binding, the prototype in avx.h,
the ABI version, and the argument checks of yuv.yuv_hdr_to_rgb_scaled that come before anything asks for a device."""
import ctypes
import os

import numpy as np
import pytest

import _rawyuv_ref as R


def test_symbol_is_exported_and_bound():
    from animal_vision_amd import _lib

    fn = _lib.lib.avx_yuv_hdr_to_rgb_scaled_u8
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    assert fn.argtypes[12] is ctypes.c_double and fn.argtypes[13] is ctypes.c_double
    assert _lib.lib.avx_abi_version() == 1
    # a NULL context is refused before anything else is looked at
    assert fn(None, 8, None, None, 1, 8, 8, 4, 4, 0, 1, 1, 1000.0, 203.0, None) == _lib.AVX_ERR_INVALID
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avx.h")).read()
    assert ("int avx_yuv_hdr_to_rgb_scaled_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int Hd, "
            "int Wd,\n                                 int full_range, int transfer, int tonemap, double peak_nits, double sdr_white, void* stream);") in hdr
    assert "#define AVX_ABI_VERSION 1" in hdr


def test_bad_arguments_raise_before_a_device_is_asked_for(monkeypatch):
    from animal_vision_amd import yuv

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(yuv, "get_context", no_device)
    H, W, fmt = 8, 8, "p010le"
    buf = np.zeros(R.frame_size(fmt, H, W), np.uint8)
    ok = dict(pix_fmt=fmt, transfer="pq")
    for Hd, Wd in ((9, 8), (8, 9), (0, 4), (4, -1)):  # enlarging on either axis, non-positive sizes
        with pytest.raises(ValueError):
            yuv.yuv_hdr_to_rgb_scaled(buf, H, W, Hd, Wd, **ok)
    for bad in (dict(pix_fmt="nv12"), dict(pix_fmt="yuv420p"), dict(pix_fmt="gray"), dict(pix_fmt="p016le"),  # 8-bit formats, no format
                dict(transfer="srgb"), dict(transfer=None), dict(tonemap="reinhard"), dict(range="tv"),
                dict(peak_nits=203.0), dict(peak_nits=100.0), dict(peak_nits=float("nan")), dict(sdr_white=0.0), dict(sdr_white=float("inf"))):
        with pytest.raises(ValueError):
            yuv.yuv_hdr_to_rgb_scaled(buf, H, W, 4, 4, **{**ok, **bad})
    with pytest.raises(ValueError):  # a payload of the wrong size
        yuv.yuv_hdr_to_rgb_scaled(buf[:-2], H, W, 4, 4, **ok)
    with pytest.raises(AssertionError, match="the device was asked for"):  # good arguments do reach the device
        yuv.yuv_hdr_to_rgb_scaled(buf, H, W, 4, 4, **ok)


def test_device_wrapper_checks_settings_and_sizes_first():
    from animal_vision_amd import yuv

    class Ctx:  # never reached: every call below is refused before the context is used
        def __getattr__(self, name):
            raise AssertionError("the device was asked for")

    class Buf:
        ptr, nbytes = 0, 1 << 20

    for kw, sizes in ((dict(transfer="pq"), (8, 8, 9, 8)), (dict(transfer="pq"), (8, 8, 8, 16)), (dict(transfer="log"), (8, 8, 4, 4)),
                      (dict(transfer="hlg", tonemap="none"), (8, 8, 4, 4)), (dict(transfer="hlg", peak_nits=100.0, sdr_white=203.0), (8, 8, 4, 4))):
        with pytest.raises(ValueError):
            yuv.yuv_hdr_to_rgb_scaled_device(Ctx(), "p010le", Buf(), Buf(), 1, *sizes, **kw)
    with pytest.raises(ValueError):
        yuv.yuv_hdr_to_rgb_scaled_device(Ctx(), "nv12", Buf(), Buf(), 1, 8, 8, 4, 4, transfer="pq")
    small = Buf()
    small.nbytes = 8
    with pytest.raises(ValueError):  # an undersized destination
        yuv.yuv_hdr_to_rgb_scaled_device(Ctx(), "p010le", Buf(), small, 1, 8, 8, 4, 4, transfer="pq")


def test_frame_pipeline_refuses_a_bad_hdr_scale_before_it_touches_the_device():
    from animal_vision_amd.pipeline import FramePipeline

    class Op:
        ctx = None

    for bad in ((161, 96), (160, 97), (0, 48), (80,)):
        with pytest.raises(ValueError):
            FramePipeline(Op(), 96, 160, io_format="yuv", pix_fmt="p010le", transfer="pq", scale=bad)
    with pytest.raises(ValueError):
        FramePipeline(Op(), 96, 160, io_format="yuv", pix_fmt="nv12", transfer="pq", scale=(80, 48))
