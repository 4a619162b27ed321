"""The XCD-aware tile order of the persistent MST++ tile kernels changes WHERE a tile is computed, never what: every kernel that takes it
returns the same bytes as under AVX_MST_TILE_ORDER=raster (the switch is read per call), on frames smaller than a tile, ragged against the
tiles, with more tiles than workgroups, in batches -- and so does a whole forward pass."""
import numpy as np
import pytest
import torch

from conftest import load_golden

# (frames, height, width): smaller than a tile; not a multiple of the tile (14 x 16, 14 x 8 and 16 x 16 pixels); two frames; more tiles than the 512 workgroups
# the largest launch of a 256-CU part takes (16 x 16: 25 x 27 = 675; 14 x 16: 25 x 30 = 750)
SHAPES = [(1, 5, 9), (1, 37, 53), (2, 45, 61), (1, 400, 420), (2, 203, 417)]


def _both_orders(monkeypatch, run):
    monkeypatch.delenv("AVX_MST_TILE_ORDER", raising=False)
    got = run()
    monkeypatch.setenv("AVX_MST_TILE_ORDER", "raster")
    want = run()
    monkeypatch.delenv("AVX_MST_TILE_ORDER", raising=False)
    torch.cuda.synchronize()
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", [32, 64, 128])
def test_attn_tail_mx_is_bit_identical_under_both_tile_orders(monkeypatch, c, shape):
    from animal_vision_amd._lib import lib
    from animal_vision_amd.ml.mst_plus_plus import _AVX, pack_dw_mfma, pack_fragments16, pad_channels

    torch.manual_seed(13 * c + shape[1] + shape[2])
    dev = torch.device("cuda")
    b, h, w = shape
    heads, real = c // 32, c // 32 * 31
    x = pad_channels(torch.randn(b, h, w, real, device=dev), (3,)).half().contiguous()
    wv = pack_fragments16(pad_channels(torch.randn(real, real, device=dev) * 0.25, (0, 1)).half().contiguous(), halfrow=True)
    gram = torch.randn(heads, 32, 32, device=dev) * 3
    nq, nk = torch.rand(c, device=dev) + 0.5, torch.rand(c, device=dev) + 0.5
    nk[31::32] = 0.0
    mp = _AVX.attn_pack_mx(gram, nq, nk, torch.rand(heads, device=dev) + 0.5, pad_channels(torch.randn(real, real, device=dev) * 0.2, (0, 1)))
    gs = _AVX.gelu_prescale()
    dw1 = pack_dw_mfma((pad_channels(torch.randn(real, 1, 3, 3, device=dev) * 0.3, (0,)).float() / gs).half())
    dw2 = pack_dw_mfma((pad_channels(torch.randn(real, 1, 3, 3, device=dev) * 0.3, (0,)).float() * gs).half())
    bias = pad_channels(torch.randn(real, device=dev), (0,)).float()
    ctx = _AVX.ctx(dev)

    def run():  # the C entry point itself: the Python wrapper takes one frame, the kernel a batch (frames that share M)
        out = torch.full_like(x, float("nan"))
        ctx._check(lib.avx_mst_attn_tail_mx(ctx._h, x.data_ptr(), wv.data_ptr(), mp.data_ptr(), dw1.data_ptr(), dw2.data_ptr(), bias.data_ptr(), out.data_ptr(), b, h, w, c,
                                            torch.cuda.current_stream(dev).cuda_stream))
        return out

    got, want = _both_orders(monkeypatch, run)
    assert not torch.isnan(want.float()).any()  # every pixel was written
    assert torch.equal(got, want)
    for i in range(b):  # and a frame of a batch equals the frame alone (the wrapper's call)
        assert torch.equal(got[i], _AVX.attn_tail_mx(x[i], wv, mp, dw1, dw2, bias))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", [32, 64, 128])
def test_ffn_fused_mx_is_bit_identical_under_both_tile_orders(monkeypatch, c, shape):
    from animal_vision_amd.ml.mst_plus_plus import _AVX, fold_layernorm, pack_dw_mfma, pack_fragments16, pad_channels

    torch.manual_seed(17 * c + shape[1] + shape[2])
    dev = torch.device("cuda")
    b, h, w = shape
    real = c // 32 * 31
    x = pad_channels(torch.randn(b, h, w, real, device=dev), (3,)).half()
    gam = pad_channels(torch.randn(real, device=dev), (0,)).float()
    bet = pad_channels(torch.randn(real, device=dev) * 0.3, (0,)).float()
    w1 = pad_channels(torch.randn(4 * real, real, device=dev) * 0.25, (0, 1)).half().t().contiguous()
    wd = pad_channels(torch.randn(4 * real, 1, 3, 3, device=dev) * 0.3, (0,)).half()
    w2 = pad_channels(torch.randn(real, 4 * real, device=dev) * 0.1, (0, 1)).half().t().contiguous()
    gs = _AVX.gelu_prescale()
    w1p, w2p, dwp = pack_fragments16(fold_layernorm(w1, gam, bet, gs).half()), pack_fragments16((w2.float() * gs).half()), pack_dw_mfma(wd)
    got, want = _both_orders(monkeypatch, lambda: _AVX.ffn_fused(x, gam, bet, w1p, None, w2p, dwpack=dwp))
    assert torch.equal(got, want)
    # the vector-unit form of the kernel walks the same order
    taps = wd.reshape(4 * c, 9).t().contiguous()
    got, want = _both_orders(monkeypatch, lambda: _AVX.ffn_fused(x, gam, bet, pack_fragments16(w1), taps, pack_fragments16(w2)))
    assert torch.equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 6, 10), (2, 38, 54), (1, 400, 420), (1, 1088, 1920)])
def test_conv3x3_lds_and_down4x4_are_bit_identical_under_both_tile_orders(monkeypatch, shape):
    """(1, 1088, 1920): 4,080 (c = 32) / 8,160 (c = 64) downsampling tiles over one workgroup per CU -- the look-ahead ring of LDS-direct loads in its steady state,
    across band crossings and past each walk's end."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX, pack_down4x4, pack_fragments16

    torch.manual_seed(shape[1] + shape[2])
    dev = torch.device("cuda")
    b, h, w = shape
    x = torch.randn(b, h, w, 32, device=dev).half()
    add = torch.randn(b, h, w, 32, device=dev).half()
    wt = (torch.randn(32, 32, 3, 3, device=dev) * 0.1).half()
    wq = torch.stack([pack_fragments16(wt[:, :, t // 3, t % 3].t().contiguous()) for t in range(9)]).contiguous()
    got, want = _both_orders(monkeypatch, lambda: _AVX.conv3x3_lds(x, wq, add))
    assert torch.equal(got, want)
    for c in (32, 64):
        xc = torch.randn(b, h, w, c, device=dev).half()
        wp = pack_down4x4((torch.randn(2 * c, c, 4, 4, device=dev) * (2.5 / c)).half())
        got, want = _both_orders(monkeypatch, lambda: _AVX.down4x4(xc, wp))
        assert torch.equal(got, want)


@pytest.mark.gpu
def test_forward_1080p_is_bit_identical_under_both_tile_orders(monkeypatch):
    from animal_vision_amd.ml import MSTPlusPlus
    from animal_vision_amd.synthetic import structured_frame

    wts = load_golden("mstpp_weights_fp16")
    model = MSTPlusPlus().load_reference_state_dict({k: torch.from_numpy(wts[k].astype(np.float32)) for k in wts.files}).eval().cuda().half()
    x = torch.from_numpy((structured_frame(3, 1080, 1920).astype(np.float32) / 255.0).transpose(2, 0, 1)[None].copy()).cuda().half()
    with torch.no_grad():
        got, want = _both_orders(monkeypatch, lambda: model(x).clone())
    assert got.shape[1] == 31 and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
