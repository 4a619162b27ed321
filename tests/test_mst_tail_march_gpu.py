"""The column-marching attention tail (avx_mst_attn_tail_mx_col / _sp_col: 28 x 8 tiles at C = 32, 14 x 14 at C = 64; two rows of v and of x and one mid row pair
carried on chip from the tile above) returns the bytes of the current kernel (avx_mst_attn_tail_mx / _sp) on the same inputs, dense and sparse: a v pixel, a mid
pixel, the projection's K order and the residual do not depend on which tile computes them.  Shapes, C = 32: a single pixel; exactly one tile; a pixel more each
way; two tiles of a column; narrower than one column block over three steps; a second block one pixel wide; two frames of 5 x 3 tiles.  C = 64: a single pixel; one
tile; a pixel more each way; two frames of 3 x 3 tiles.  max_workgroups 0 (one tile per workgroup at these sizes: every tile behind its own priming step) and a few
workgroups, so that runs carry rows down a column, break in the middle of one, and go on across columns and frames."""
import numpy as np
import pytest
import torch

from conftest import load_golden

CASES = [(32, s, (0, 1, 2, 5)) for s in [(1, 1, 1), (1, 8, 28), (1, 9, 29), (1, 16, 28), (1, 24, 13), (1, 10, 15), (2, 37, 61)]] + [
    (64, s, (0, 1, 3)) for s in [(1, 1, 1), (1, 14, 14), (1, 15, 15), (2, 31, 33)]
]


@pytest.mark.gpu
@pytest.mark.parametrize("c,shape,caps", CASES)
def test_tail_march_is_bit_identical_to_the_current_kernel(c, shape, caps):
    from animal_vision_amd._lib import lib
    from animal_vision_amd.ml.mst_plus_plus import _AVX, pack_dw_mfma, pack_dw_smfmac, pack_fragments16, pad_channels

    torch.manual_seed(23 * c + shape[1] + shape[2])
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
    w1 = (pad_channels(torch.randn(real, 1, 3, 3, device=dev) * 0.3, (0,)).float() / gs).half()
    w2 = (pad_channels(torch.randn(real, 1, 3, 3, device=dev) * 0.3, (0,)).float() * gs).half()
    bias = pad_channels(torch.randn(real, device=dev), (0,)).float()
    ctx = _AVX.ctx(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for sparse in (False, True):
        pk = pack_dw_smfmac if sparse else pack_dw_mfma
        dw1, dw2 = pk(w1), pk(w2)
        args = (ctx._h, x.data_ptr(), wv.data_ptr(), mp.data_ptr(), dw1.data_ptr(), dw2.data_ptr(), bias.data_ptr())
        want = torch.full_like(x, float("nan"))
        ctx._check((lib.avx_mst_attn_tail_sp if sparse else lib.avx_mst_attn_tail_mx)(*args, want.data_ptr(), b, h, w, c, st))
        assert torch.isfinite(want.float()).all()
        fn = lib.avx_mst_attn_tail_sp_col if sparse else lib.avx_mst_attn_tail_mx_col
        for cap in caps:
            got = torch.full_like(x, float("nan"))  # the C entry point itself, into a poisoned buffer: every pixel must be written
            ctx._check(fn(*args, got.data_ptr(), b, h, w, c, cap, st))
            assert torch.equal(got, want), (c, shape, sparse, cap, int((got != want).sum()))
        # and the wrapper's route (one frame)
        assert torch.equal(_AVX.attn_tail_mx(x[0], wv, mp, dw1, dw2, bias, sparse=sparse, march=True, max_workgroups=caps[-1]), want[0])


@pytest.mark.gpu
def test_tail_march_refuses_what_it_is_not_built_for():
    from animal_vision_amd._lib import lib
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    dev = torch.device("cuda")
    ctx = _AVX.ctx(dev)
    t = torch.zeros(1 << 16, device=dev, dtype=torch.float16)
    o = torch.zeros_like(t)
    f = torch.zeros(128, device=dev)
    args = (ctx._h, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), f.data_ptr(), o.data_ptr(), 1, 4, 4)
    for fn in (lib.avx_mst_attn_tail_mx_col, lib.avx_mst_attn_tail_sp_col):
        assert fn(*args, 128, 0, None) != 0  # C = 128 stays on the 14 x 8 kernel
        assert fn(*args, 32, -1, None) != 0
        assert fn(*args, 64, -1, None) != 0


@pytest.mark.gpu
def test_forward_64x64_is_bit_identical_with_the_tail_march_on_and_off(monkeypatch):
    from animal_vision_amd.ml import MSTPlusPlus
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    from animal_vision_amd.synthetic import structured_frame

    wts = load_golden("mstpp_weights_fp16")
    model = MSTPlusPlus().load_reference_state_dict({k: torch.from_numpy(wts[k].astype(np.float32)) for k in wts.files}).eval().cuda().half()
    x = torch.from_numpy((structured_frame(3, 64, 64).astype(np.float32) / 255.0).transpose(2, 0, 1)[None].copy()).cuda().half()
    with torch.no_grad():
        monkeypatch.setattr(_AVX, "_tail_march", True)
        monkeypatch.setattr(_AVX, "TAIL_MARCH_C", (32, 64))  # both widths, whatever the route keeps
        got = model(x).clone()
        monkeypatch.setattr(_AVX, "_tail_march", False)
        want = model(x).clone()
    torch.cuda.synchronize()
    assert got.shape[1] == 31 and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
