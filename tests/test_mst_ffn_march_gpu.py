"""The column-marching FeedForward kernel (avx_mst_ffn_fused_mx_col / _sp_col: 16 x 14 tiles, two halo rows carried on chip from the tile above) returns the bytes
of the 16-row kernel (_AVX.ffn_fused) on the same inputs, dense and sparse: a hidden pixel's value, the second GEMM's K order and the residual do not depend on
which tile computes them.  Shapes: a single pixel; exactly one tile; a pixel more than a tile each way; two tiles of a column; a third tile of one row in a narrow
column; two frames of 4 x 3 tiles.  max_workgroups 0 (one tile per workgroup at these sizes: every tile a segment start) and a few workgroups, so that runs carry
rows down a column, break in the middle of one, and go on across columns and frames."""
import numpy as np
import pytest
import torch

from conftest import load_golden

CASES = [(32, s, (0, 1, 2, 5)) for s in [(1, 1, 1), (1, 14, 16), (1, 15, 17), (1, 28, 16), (1, 29, 5), (2, 45, 37)]] + [(64, s, (0, 1, 3)) for s in [(1, 1, 1), (2, 31, 19)]]


@pytest.mark.gpu
@pytest.mark.parametrize("c,shape,caps", CASES)
def test_ffn_march_is_bit_identical_to_the_16_row_kernel(c, shape, caps):
    from animal_vision_amd._lib import lib
    from animal_vision_amd.ml.mst_plus_plus import _AVX, fold_layernorm, pack_dw_mfma, pack_dw_smfmac, pack_fragments16, pad_channels

    torch.manual_seed(19 * c + shape[1] + shape[2])
    dev = torch.device("cuda")
    b, h, w = shape
    real = c // 32 * 31
    x = pad_channels(torch.randn(b, h, w, real, device=dev), (3,)).half().contiguous()
    gam = pad_channels(torch.randn(real, device=dev), (0,)).float()
    bet = pad_channels(torch.randn(real, device=dev) * 0.3, (0,)).float()
    w1 = pad_channels(torch.randn(4 * real, real, device=dev) * 0.25, (0, 1)).half().t().contiguous()
    wd = pad_channels(torch.randn(4 * real, 1, 3, 3, device=dev) * 0.3, (0,)).half()
    w2 = pad_channels(torch.randn(real, 4 * real, device=dev) * 0.1, (0, 1)).half().t().contiguous()
    gs = _AVX.gelu_prescale()
    w1p, w2p = pack_fragments16(fold_layernorm(w1, gam, bet, gs).half()), pack_fragments16((w2.float() * gs).half())
    ctx = _AVX.ctx(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for sparse in (False, True):
        dwp = pack_dw_smfmac(wd) if sparse else pack_dw_mfma(wd)
        want = _AVX.ffn_fused(x, gam, bet, w1p, None, w2p, dwpack=dwp, sparse=sparse)
        assert torch.isfinite(want.float()).all()
        fn = lib.avx_mst_ffn_fused_sp_col if sparse else lib.avx_mst_ffn_fused_mx_col
        for cap in caps:
            got = torch.full_like(x, float("nan"))  # the C entry point itself, into a poisoned buffer: every pixel must be written
            ctx._check(fn(ctx._h, x.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-5, w1p.data_ptr(), dwp.data_ptr(), w2p.data_ptr(), got.data_ptr(), b, h, w, c, cap, st))
            assert torch.equal(got, want), (c, shape, sparse, cap, int((got != want).sum()))
        # and the wrapper's route
        assert torch.equal(_AVX.ffn_fused(x, gam, bet, w1p, None, w2p, dwpack=dwp, sparse=sparse, march=True, max_workgroups=caps[-1]), want)


@pytest.mark.gpu
def test_ffn_march_refuses_what_it_is_not_built_for():
    from animal_vision_amd._lib import lib
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    dev = torch.device("cuda")
    ctx = _AVX.ctx(dev)
    t = torch.zeros(1 << 16, device=dev, dtype=torch.float16)
    o = torch.zeros_like(t)
    f = torch.zeros(128, device=dev)
    args = (ctx._h, t.data_ptr(), f.data_ptr(), f.data_ptr(), 1e-5, t.data_ptr(), t.data_ptr(), t.data_ptr(), o.data_ptr(), 1, 4, 4)
    for fn in (lib.avx_mst_ffn_fused_mx_col, lib.avx_mst_ffn_fused_sp_col):
        assert fn(*args, 128, 0, None) != 0  # C = 128 stays on the 16-row kernel
        assert fn(*args, 32, -1, None) != 0


@pytest.mark.gpu
def test_forward_64x64_is_bit_identical_with_the_march_on_and_off(monkeypatch):
    from animal_vision_amd.ml import MSTPlusPlus
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    from animal_vision_amd.synthetic import structured_frame

    wts = load_golden("mstpp_weights_fp16")
    model = MSTPlusPlus().load_reference_state_dict({k: torch.from_numpy(wts[k].astype(np.float32)) for k in wts.files}).eval().cuda().half()
    x = torch.from_numpy((structured_frame(3, 64, 64).astype(np.float32) / 255.0).transpose(2, 0, 1)[None].copy()).cuda().half()
    with torch.no_grad():
        monkeypatch.setattr(_AVX, "_ffn_march", True)
        got = model(x).clone()
        monkeypatch.setattr(_AVX, "_ffn_march", False)
        want = model(x).clone()
    torch.cuda.synchronize()
    assert got.shape[1] == 31 and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
