"""The decoder upsampling on K = 16 MFMAs (csrc/mst_mfma.hip::k_mst_convt2x2_16: avx_mst_convt2x2_fuse16, avx_mst_convt2x2_fuse16_gram) against
torch, against the K = 8 kernels it stands beside, and against the standalone Gram pass its epilogue replaces.  Shapes: those of the K = 8
kernels' tests, plus (1, 33, 100) -- a partial last wave-tile in every row -- and (1, 40, 64), more wave-tiles than one workgroup takes."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

SHAPES = [(64, (2, 5, 37)), (128, (1, 4, 32)), (64, (1, 1, 1)), (64, (1, 33, 100)), (128, (1, 33, 100)), (64, (1, 40, 64)), (128, (1, 40, 64))]


def _packs(w_taps, wskip=None):
    """Four (c, c/2) tap matrices (and the skip half of the fusion conv) in both fragment formats: (K = 8, K = 16)."""
    from animal_vision_amd.ml.mst_plus_plus import pack_fragments, pack_fragments16

    p8 = torch.stack([pack_fragments(w.contiguous(), True) for w in w_taps]).contiguous()
    p16 = torch.stack([pack_fragments16(w.contiguous(), halfrow=True) for w in w_taps]).contiguous()
    if wskip is None:
        return p8, p16
    return p8, p16, pack_fragments(wskip.contiguous(), True), pack_fragments16(wskip.contiguous(), halfrow=True)


@pytest.mark.parametrize("c,shape", SHAPES)
def test_mst_convt2x2_16_matches_torch_and_the_k8_kernel(c, shape):
    """avx_mst_convt2x2_fuse16 without skip vs F.conv_transpose2d(kernel 2, stride 2) + bias; the K = 8 kernel on the same inputs is held to
    the same tolerance (the two may sum a pixel's products in another order), the largest difference between the two is printed."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    import torch.nn.functional as F

    torch.manual_seed(c + shape[2])
    dev = torch.device("cuda")
    b, h, w = shape
    x = torch.randn(b, h, w, c, device=dev).half()
    wt = (torch.randn(c, c // 2, 2, 2, device=dev) * 0.1).half()
    bias = torch.randn(c // 2, device=dev)
    p8, p16 = _packs([wt[:, :, t // 2, t % 2] for t in range(4)])
    got = _AVX.convt2x2_16(x, p16, bias)
    old = _AVX.convt2x2(x, p8, bias)
    ref = F.conv_transpose2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, stride=2).permute(0, 2, 3, 1)
    assert got.shape == ref.shape
    print(f"convt2x2 K=16 vs K=8, c={c} {shape}: max |diff| {float((got.float() - old.float()).abs().max()):.3e}")
    torch.testing.assert_close(got.float(), ref, rtol=4e-3, atol=8e-3)
    torch.testing.assert_close(old.float(), ref, rtol=4e-3, atol=8e-3)
    assert torch.equal(_AVX.convt2x2_16(x, p16, bias), got)


def _fused_case(c, shape, seed):
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    b, h, w = shape
    ch = c // 2
    x = torch.randn(b, h, w, c, device=dev).half()
    skip = torch.randn(b, 2 * h, 2 * w, ch, device=dev).half()
    wt = (torch.randn(c, ch, 2, 2, device=dev) * 0.1).half()
    bias = torch.randn(ch, device=dev) * 0.2
    wf = (torch.randn(ch, 2 * ch, device=dev) * 0.1).half().t().contiguous()  # (2 ch, ch): y = cat([up, skip]) @ wf
    taps = [(wt[:, :, t // 2, t % 2].float() @ wf[:ch].float()).half() for t in range(4)]
    gb = (bias.float() @ wf[:ch].float()).contiguous()
    return x, skip, wt, bias, wf, taps, gb


@pytest.mark.parametrize("c,shape", SHAPES)
def test_mst_convt2x2_16_fused_with_the_fusion_conv_matches_torch_and_the_k8_kernel(c, shape):
    """avx_mst_convt2x2_fuse16 with skip vs ConvTranspose2d(2, stride 2) -> cat([up, skip]) -> 1x1 conv in torch, the conv's `up` half folded into
    the taps on the host as ml/mst_plus_plus.py does; the K = 8 kernel likewise."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    import torch.nn.functional as F

    x, skip, wt, bias, wf, taps, gb = _fused_case(c, shape, c + shape[2] + 7)
    ch = c // 2
    p8, p16, s8, s16 = _packs(taps, wf[ch:])
    got = _AVX.convt2x2_16(x, p16, gb, skip, s16)
    old = _AVX.convt2x2(x, p8, gb, skip, s8)
    up = F.conv_transpose2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, stride=2).permute(0, 2, 3, 1)
    ref = torch.cat([up, skip.float()], dim=-1) @ wf.float()
    assert got.shape == ref.shape
    print(f"convt2x2_fuse K=16 vs K=8, c={c} {shape}: max |diff| {float((got.float() - old.float()).abs().max()):.3e}")
    torch.testing.assert_close(got.float(), ref, rtol=6e-3, atol=1.2e-2)
    torch.testing.assert_close(old.float(), ref, rtol=6e-3, atol=1.2e-2)


@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("shape", [(2, 5, 37), (1, 1, 1), (1, 40, 64), (1, 33, 100)])
def test_mst_convt2x2_16_with_the_gram_pass_as_epilogue(c, shape):
    """avx_mst_convt2x2_fuse16_gram vs avx_mst_convt2x2_fuse16 followed by avx_mst_qkv_gram16 on its output: same output bits; per head, Gram
    matrix and column norms equal up to the order of the float32 sums (q and k themselves are formed from the same operands in both)."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX, pack_fragments16, pack_qkv16, pad_channels

    torch.manual_seed(shape[2] + 77 + c)
    dev = torch.device("cuda")
    b, h, w = shape
    ch, heads = c // 2, c // 64
    g31 = 31 * heads  # real channels of the output level
    x = pad_channels(torch.randn(b, h, w, 2 * g31, device=dev), (3,)).half()
    skip = pad_channels(torch.randn(b, 2 * h, 2 * w, g31, device=dev), (3,)).half()
    wt = torch.stack([pack_fragments16(pad_channels(torch.randn(2 * g31, g31, device=dev) * 0.1, (0, 1)).half().contiguous(), halfrow=True) for _ in range(4)]).contiguous()
    ws = pack_fragments16(pad_channels(torch.randn(g31, g31, device=dev) * 0.2, (0, 1)).half().contiguous(), halfrow=True)
    bias = pad_channels(torch.randn(g31, device=dev) * 0.1, (0,)).float()
    wqkv = torch.cat([pad_channels(torch.randn(g31, g31, device=dev) * 0.2, (0, 1)).half() for _ in range(3)], 0).t().contiguous()
    assert x.shape[-1] == c and wqkv.shape == (ch, 3 * ch)
    ref = _AVX.convt2x2_16(x, wt, bias, skip, ws)
    _, g_ref, nq_ref, nk_ref = _AVX.qkv_gram(ref.reshape(b, 4 * h * w, ch), pack_qkv16(wqkv), heads, want_v=False, k16=True)
    out, g, nq, nk = _AVX.convt2x2_16_gram(x, wt, bias, skip, ws, pack_qkv16(wqkv))
    assert torch.equal(out, ref)
    assert g.shape == g_ref.shape == (b, heads, 32, 32) and nq.shape == nq_ref.shape == (b, ch)
    n = 4 * h * w
    for hd in range(heads):
        torch.testing.assert_close(g[:, hd], g_ref[:, hd], rtol=1e-4, atol=1e-3 * (n / 64) ** 0.5)
        torch.testing.assert_close(nq[:, 32 * hd:32 * hd + 32], nq_ref[:, 32 * hd:32 * hd + 32], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(nk[:, 32 * hd:32 * hd + 32], nk_ref[:, 32 * hd:32 * hd + 32], rtol=1e-5, atol=1e-5)


def test_forward_256_with_and_without_the_k16_upsampling():
    """One 256^2 forward pass through the route of AVX_MST_NO_CONVT16=1 (the K = 8 upsampling kernels, the decoder's 62-channel block running its
    own Gram launch) and through the default route: two float16 evaluations of one network, held to the yardstick of
    tests/test_mstpp.py::test_forward_4k_fused_kernels_vs_library_ops (mean <= 2.2e-4, max <= 6e-3)."""
    from animal_vision_amd.ml import MSTPlusPlusPredictor
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    from animal_vision_amd.synthetic import structured_frame

    w = load_golden("mstpp_weights_fp16")
    sd = {k: torch.from_numpy(w[k].astype(np.float32)) for k in w.files}
    pred = MSTPlusPlusPredictor(sd, half=True)
    frame = torch.from_numpy(structured_frame(12, 256, 256)).cuda()
    was = _AVX._convt16
    try:
        _AVX._convt16 = True
        got = pred.predict_device_nhwc(frame).clone()
        _AVX._convt16 = False
        ref = pred.predict_device_nhwc(frame).clone()
    finally:
        _AVX._convt16 = was
    torch.cuda.synchronize()
    assert got.shape == (256, 256, 32) and bool(torch.isfinite(got).all())
    d = (got.float() - ref.float()).abs()
    mean, mx = float(d.mean()), float(d.max())
    print(f"256^2 forward, K = 16 upsampling vs K = 8: mean {mean:.3e}, max {mx:.3e}")
    assert mean <= 2.2e-4 and mx <= 6e-3, (mean, mx)
    assert float(got[..., :31].float().std()) > 1e-2
