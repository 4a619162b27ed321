"""GPU: the two-instruction depthwise units (one dense v_mfma_f32_16x16x32_f16 + one 2:4-sparse v_smfmac_f32_16x16x64_f16) of
avx_mst_ffn_fused_sp and avx_mst_attn_tail_sp, held to the comparisons and tolerances of tests/test_mstpp.py's
test_mst_ffn_fused_matches_torch_ops / test_mst_attn_tail_mx_matches_torch_ops, against the dense entry points on the same inputs within
those tolerances, and through one forward pass with the route switched on and off."""
import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.mark.gpu
@pytest.mark.parametrize("c,shape", [(32, (1, 16, 16)), (32, (2, 37, 53)), (32, (1, 5, 70)), (32, (1, 1, 1)), (64, (1, 16, 32)), (64, (2, 21, 19)), (64, (1, 1, 1)),
                                     (128, (1, 7, 37))])
def test_mst_ffn_fused_sp_matches_torch_ops_and_the_dense_form(c, shape):
    from animal_vision_amd.ml.mst_plus_plus import _AVX, fold_layernorm, pack_dw_mfma, pack_dw_smfmac, pack_fragments16, pad_channels
    import torch.nn.functional as F

    torch.manual_seed(c + shape[1] * 7 + shape[2])
    dev = torch.device("cuda")
    b, h, w = shape
    real = c // 32 * 31
    x = pad_channels(torch.randn(b, h, w, real, device=dev), (3,)).half()
    gam = pad_channels(torch.randn(real, device=dev), (0,)).float()
    bet = pad_channels(torch.randn(real, device=dev) * 0.3, (0,)).float()
    w1 = pad_channels(torch.randn(4 * real, real, device=dev) * 0.25, (0, 1)).half().t().contiguous()   # (c, 4c)
    wd = pad_channels(torch.randn(4 * real, 1, 3, 3, device=dev) * 0.3, (0,)).half()                     # (4c, 1, 3, 3)
    w2 = pad_channels(torch.randn(real, 4 * real, device=dev) * 0.1, (0, 1)).half().t().contiguous()    # (4c, c)
    gs = _AVX.gelu_prescale()
    w1p, w2p = pack_fragments16(fold_layernorm(w1, gam, bet, gs).half()), pack_fragments16((w2.float() * gs).half())
    got = _AVX.ffn_fused(x, gam, bet, w1p, None, w2p, dwpack=pack_dw_smfmac(wd), sparse=True)
    dense = _AVX.ffn_fused(x, gam, bet, w1p, None, w2p, dwpack=pack_dw_mfma(wd))
    other = _AVX.ffn_fused(x, gam, bet, pack_fragments16(w1), wd.reshape(4 * c, 9).t().contiguous(), pack_fragments16(w2))
    print(f"c {c} {shape}: sparse vs dense max {float((got.float() - dense.float()).abs().max()):.3e}, differing {int((got != dense).sum())} of {got.numel()}")
    torch.testing.assert_close(got.float(), other.float(), rtol=3e-3, atol=9e-3)
    assert float((got.float() - other.float()).abs().mean()) < 5e-4 * (c / 32) ** 0.75
    idx = torch.tensor([i for i in range(c) if i % 32 != 31], device=dev)
    ln = torch.zeros(b, h, w, c, device=dev)
    ln[..., idx] = F.layer_norm(x.float()[..., idx], (real,), gam[idx], bet[idx])
    hid = F.gelu((ln.half().reshape(-1, c) @ w1).float()).half().reshape(b, h, w, 4 * c)
    conv = F.conv2d(hid.float().permute(0, 3, 1, 2), wd.float(), padding=1, groups=4 * c).permute(0, 2, 3, 1).half()
    ref = x.float() + (F.gelu(conv.float()).half().reshape(-1, 4 * c) @ w2).float().reshape(b, h, w, c)
    assert got.shape == x.shape and got.data_ptr() != x.data_ptr()
    torch.testing.assert_close(got.float(), ref, rtol=4e-3, atol=1.2e-2)
    assert float((got.float() - ref).abs().mean()) < (2.0e-3 if c == 128 else 1.5e-3)
    assert torch.equal(got[..., 31::32], x[..., 31::32])
    torch.testing.assert_close(got.float(), dense.float(), rtol=4e-3, atol=1.2e-2)  # the same products in another summation order


@pytest.mark.gpu
@pytest.mark.parametrize("c,hw", [(32, (16, 14)), (32, (37, 53)), (32, (1, 1)), (64, (21, 19)), (64, (3, 2)), (128, (9, 17))])
def test_mst_attn_tail_sp_matches_torch_ops_and_the_dense_form(c, hw):
    from animal_vision_amd.ml.mst_plus_plus import _AVX, pack_dw_mfma, pack_dw_smfmac, pack_fragments16, pad_channels
    import torch.nn.functional as F

    torch.manual_seed(11 * c + hw[0] * 3 + hw[1])
    dev = torch.device("cuda")
    h, w = hw
    heads, real = c // 32, c // 32 * 31
    x = pad_channels(torch.randn(h, w, real, device=dev), (2,)).half()
    wv = pad_channels(torch.randn(real, real, device=dev) * 0.25, (0, 1)).half()  # (K = in, N = out): v = x @ wv
    v = (x.reshape(-1, c) @ wv).reshape(h, w, c).contiguous()
    gram = torch.randn(heads, 32, 32, device=dev) * 3
    nq, nk = torch.rand(c, device=dev) + 0.5, torch.rand(c, device=dev) + 0.5
    nk[31::32] = 0.0
    resc = torch.rand(heads, device=dev) + 0.5
    wpt = pad_channels(torch.randn(real, real, device=dev) * 0.2, (0, 1))
    bias = pad_channels(torch.randn(real, device=dev), (0,)).float()
    w1 = pad_channels(torch.randn(real, 1, 3, 3, device=dev) * 0.3, (0,)).half()
    w2 = pad_channels(torch.randn(real, 1, 3, 3, device=dev) * 0.3, (0,)).half()
    gs = _AVX.gelu_prescale()
    wvp, mp = pack_fragments16(wv.contiguous(), halfrow=True), _AVX.attn_pack_mx(gram, nq, nk, resc, wpt)
    w1s, w2s = (w1.float() / gs).half(), (w2.float() * gs).half()
    got = _AVX.attn_tail_mx(x, wvp, mp, pack_dw_smfmac(w1s), pack_dw_smfmac(w2s), bias, sparse=True)
    dense = _AVX.attn_tail_mx(x, wvp, mp, pack_dw_mfma(w1s), pack_dw_mfma(w2s), bias)
    print(f"c {c} {hw}: sparse vs dense max {float((got.float() - dense.float()).abs().max()):.3e}, differing {int((got != dense).sum())} of {got.numel()}")
    assert got.shape == x.shape and got.data_ptr() != x.data_ptr()
    attn = gram / (nk.clamp_min(1e-12).reshape(heads, 32, 1) * nq.clamp_min(1e-12).reshape(heads, 1, 32)) * resc.reshape(heads, 1, 1)
    attn[..., 31:] = float("-inf")
    attn = attn.softmax(dim=-1)
    M = torch.matmul(attn.transpose(-2, -1), wpt.reshape(heads, 32, c)).reshape(c, c).half()
    mid = F.gelu(F.conv2d(v.float().permute(2, 0, 1)[None], w1.float(), padding=1, groups=c)).half().float()
    pe = F.conv2d(mid, w2.float(), padding=1, groups=c)[0].permute(1, 2, 0)
    ref = (v.reshape(-1, c) @ M).float().reshape(h, w, c) + bias + pe + x.float()
    torch.testing.assert_close(got.float(), ref, rtol=4e-3, atol=1.5e-2)
    assert float((got.float() - ref).abs().mean()) < 2e-3
    torch.testing.assert_close(got.float(), dense.float(), rtol=4e-3, atol=1.5e-2)


@pytest.mark.gpu
def test_forward_256_with_the_sparse_route_on_and_off():
    """The smallest fixture of test_forward_fp16_large_frames_vs_reference (256 x 256) through the whole network, the sparse route on (the
    default) and off: both runs meet that test's bound, and the two outputs differ by float16 roundings only."""
    from animal_vision_amd.ml import MSTPlusPlus
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    from animal_vision_amd.synthetic import structured_frame

    wt = load_golden("mstpp_weights_fp16")
    sd = {k: torch.from_numpy(wt[k].astype(np.float32)) for k in wt.files}
    g = load_golden("mstpp_large")
    yard = g["autocast_err_256"]
    seed, h, w = (int(v) for v in g["seed_256"])
    x = torch.from_numpy((structured_frame(seed, h, w).astype(np.float32) / 255.0).transpose(2, 0, 1)[None].copy()).cuda().half()
    ref = g["y_256"].astype(np.float32)
    floor = 2.5e-4  # the float16 container of the 256x256 fixture
    was, ys = _AVX._dwsp, {}
    try:
        for on in (True, False):
            _AVX._dwsp = on
            m = MSTPlusPlus().load_reference_state_dict(sd).eval().cuda().half()  # a fresh model: its prepared weights follow the switch
            ys[on] = m(x).float().cpu().numpy()[0]
            assert any(".dwsp" in k for k in m._prepared) == on  # the switch reaches the weight packs (widths that keep the dense form prepare pack_dw_mfma's either way)
            d = np.abs(ys[on].astype(np.float64) - ref.astype(np.float64))
            mx, mean, rms = float(d.max()), float(d.mean()), float(np.sqrt((d ** 2).mean()))
            msg = f"256, sparse {on}: max {mx:.3e} (reference autocast {yard[0]:.3e}), mean {mean:.3e} ({yard[1]:.3e}), rms {rms:.3e} ({yard[2]:.3e})"
            print(msg)
            assert mx <= 2 * yard[0] + floor and mean <= 2 * yard[1] + floor / 4 and rms <= 2 * yard[2] + floor / 4, msg
    finally:
        _AVX._dwsp = was
    print(f"sparse on vs off: max {float(np.abs(ys[True] - ys[False]).max()):.3e}")
