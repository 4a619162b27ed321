"""The fused decoder upsampling with whole-line memory accesses (csrc/mst_mfma.hip::k_mst_convt2x2_16_ln: avx_mst_convt2x2_fuse16_ln,
avx_mst_convt2x2_fuse16_gram_ln) against the K = 16 kernel it stands beside (k_mst_convt2x2_16) on the same inputs: the same output bits.
Shapes (B, H, W of the input): those of tests/test_mst_convt16_gpu.py, plus (1, 3, 31) and (1, 2, 33) -- one pixel short of and one pixel past a
wave-tile -- and (2, 3, 8), rows shorter than one prefetched run with the batch boundary inside a workgroup's walk.  The kernel runs one workgroup of NW waves per CU
(NW = 16, 12 with the epilogue, at C = 64; 8 at C = 128) and a wave walks tiles g, g + waves, ...: LONG gives every wave of a 256-CU part more than one tile,
so the request for the next tile, the hand-over of the prefetched x, the carries of the walk and the counted waits of the steady state run under torch.equal --
whole tiles (W = 1024) and a partial last tile in every row (W = 1000)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

HWS = [(2, 5, 37), (1, 4, 32), (1, 1, 1), (1, 33, 100), (1, 40, 64), (1, 3, 31), (1, 2, 33), (2, 3, 8)]
LONG = [(64, (1, 136, 1024)), (64, (1, 136, 1000)), (128, (1, 72, 1024)), (128, (1, 72, 1000))]  # 4352 > 256 * 16 and 2304 > 256 * 8 wave-tiles
CASES = [(c, shape) for c in (64, 128) for shape in HWS] + LONG


def _case(c, shape, seed):
    """Inputs of the fused step in the K = 16 fragment format, and the block's q / k weights: 31 real channels per head, as the network has them."""
    from animal_vision_amd.ml.mst_plus_plus import pack_fragments16, pack_qkv16, pad_channels

    torch.manual_seed(seed)
    dev = torch.device("cuda")
    b, h, w = shape
    ch, heads = c // 2, c // 64
    g31 = 31 * heads
    x = pad_channels(torch.randn(b, h, w, 2 * g31, device=dev), (3,)).half()
    skip = pad_channels(torch.randn(b, 2 * h, 2 * w, g31, device=dev), (3,)).half()
    wt = torch.stack([pack_fragments16(pad_channels(torch.randn(2 * g31, g31, device=dev) * 0.1, (0, 1)).half().contiguous(), halfrow=True) for _ in range(4)]).contiguous()
    ws = pack_fragments16(pad_channels(torch.randn(g31, g31, device=dev) * 0.2, (0, 1)).half().contiguous(), halfrow=True)
    bias = pad_channels(torch.randn(g31, device=dev) * 0.1, (0,)).float()
    wqkv = torch.cat([pad_channels(torch.randn(g31, g31, device=dev) * 0.2, (0, 1)).half() for _ in range(3)], 0).t().contiguous()
    assert x.shape[-1] == c and skip.shape[-1] == ch
    return x, skip, wt, ws, bias, pack_qkv16(wqkv)


@pytest.mark.parametrize("c,shape", CASES)
def test_whole_line_form_writes_the_k16_kernels_bits(c, shape):
    """Fused, and fused with the Gram epilogue: `out` is torch.equal to k_mst_convt2x2_16's.  At C = 128 walk and geometry are the K = 16 kernel's (the
    same workgroups of 8 waves, the same tiles per wave, the same tap order): Gram matrix and norms are torch.equal too.  At C = 64 one workgroup of 12
    waves per CU sums what four workgroups of 4 summed, so the partials are grouped differently: there they take the tolerances of
    tests/test_mst_convt16_gpu.py::test_mst_convt2x2_16_with_the_gram_pass_as_epilogue (the order of the float32 sums)."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    x, skip, wt, ws, bias, wqk = _case(c, shape, 13 * c + shape[1] + 5 * shape[2])
    b, h, w = shape
    heads = c // 64
    ref = _AVX.convt2x2_16(x, wt, bias, skip, ws)
    got = _AVX.convt2x2_16(x, wt, bias, skip, ws, lines=True)
    assert got.shape == ref.shape == (b, 2 * h, 2 * w, c // 2)
    assert torch.equal(got, ref)
    ref_g, g_ref, nq_ref, nk_ref = _AVX.convt2x2_16_gram(x, wt, bias, skip, ws, wqk)
    out, g, nq, nk = _AVX.convt2x2_16_gram(x, wt, bias, skip, ws, wqk, lines=True)
    assert torch.equal(ref_g, ref) and torch.equal(out, ref)
    n = 4 * h * w
    for hd in range(heads):
        sl = slice(32 * hd, 32 * hd + 32)
        print(f"c={c} {shape} head {hd}: max |gram diff| {float((g[:, hd] - g_ref[:, hd]).abs().max()):.3e}, max |nq diff| {float((nq[:, sl] - nq_ref[:, sl]).abs().max()):.3e}")
        if c == 128:
            assert torch.equal(g[:, hd], g_ref[:, hd]) and torch.equal(nq[:, sl], nq_ref[:, sl]) and torch.equal(nk[:, sl], nk_ref[:, sl])
            continue
        torch.testing.assert_close(g[:, hd], g_ref[:, hd], rtol=1e-4, atol=1e-3 * (n / 64) ** 0.5)
        torch.testing.assert_close(nq[:, sl], nq_ref[:, sl], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(nk[:, sl], nk_ref[:, sl], rtol=1e-5, atol=1e-5)
    out2, g2, nq2, nk2 = _AVX.convt2x2_16_gram(x, wt, bias, skip, ws, wqk, lines=True)
    assert torch.equal(out2, out) and torch.equal(g2, g) and torch.equal(nq2, nq) and torch.equal(nk2, nk)  # run to run


def _guarded(t, pad, sentinel):
    """A copy of t in the middle of a buffer filled with `sentinel` (int16 bits): (buffer as int16, the view)."""
    n = t.numel()
    buf = torch.full((n + 2 * pad,), sentinel, dtype=torch.int16, device=t.device)
    view = buf[pad:pad + n].view(torch.float16).view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 31), (1, 2, 33)])
def test_whole_line_form_stays_inside_its_tensors(c, shape):
    """`out` is a view into the middle of a larger buffer, x and skip have NaN neighbours: after the launch every byte around `out` is what it was, and
    the output equals the K = 16 kernel's on the plain tensors -- nothing from outside x or skip reached a real pixel."""
    from animal_vision_amd._lib import lib
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    x, skip, wt, ws, bias, wqk = _case(c, shape, 7 * c + shape[2])
    b, h, w = shape
    ch, heads = c // 2, c // 64
    ref = _AVX.convt2x2_16(x, wt, bias, skip, ws)
    pad, nan16, mark = 8192, 0x7E00, 0x5A5A
    _, xg = _guarded(x, pad, nan16)
    _, sg = _guarded(skip, pad, nan16)
    ctx = _AVX.ctx(x.device)
    st = torch.cuda.current_stream(x.device).cuda_stream
    for gram in (False, True):
        obuf, og = _guarded(torch.zeros_like(ref), pad, mark)
        if gram:
            g = torch.empty((heads, 32, 32), dtype=torch.float32, device=x.device)
            nq = torch.empty((ch,), dtype=torch.float32, device=x.device)
            nk = torch.empty((ch,), dtype=torch.float32, device=x.device)
            ctx._check(lib.avx_mst_convt2x2_fuse16_gram_ln(ctx._h, xg.data_ptr(), wt.data_ptr(), bias.data_ptr(), sg.data_ptr(), ws.data_ptr(), og.data_ptr(), h, w, c, heads,
                                                           wqk.data_ptr(), g.data_ptr(), nq.data_ptr(), nk.data_ptr(), st))
            assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(nq).all()) and bool(torch.isfinite(nk).all())
        else:
            ctx._check(lib.avx_mst_convt2x2_fuse16_ln(ctx._h, xg.data_ptr(), wt.data_ptr(), bias.data_ptr(), sg.data_ptr(), ws.data_ptr(), og.data_ptr(), b, h, w, c, st))
        torch.cuda.synchronize()
        assert bool((obuf[:pad] == mark).all()) and bool((obuf[pad + ref.numel():] == mark).all()), "a store outside out"
        assert torch.equal(og, ref)


def _forward_pair(setup):
    from animal_vision_amd.ml import MSTPlusPlusPredictor
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    from animal_vision_amd.synthetic import structured_frame

    w = load_golden("mstpp_weights_fp16")
    sd = {k: torch.from_numpy(w[k].astype(np.float32)) for k in w.files}
    pred = MSTPlusPlusPredictor(sd, half=True)
    frame = torch.from_numpy(structured_frame(12, 256, 256)).cuda()
    was = _AVX._convt_lines, _AVX.CONVT_LINES_C, _AVX.CONVT_LINES_GRAM_C
    try:
        setup(_AVX)
        _AVX._convt_lines = True
        got = pred.predict_device_nhwc(frame).clone()
        _AVX._convt_lines = False
        ref = pred.predict_device_nhwc(frame).clone()
    finally:
        _AVX._convt_lines, _AVX.CONVT_LINES_C, _AVX.CONVT_LINES_GRAM_C = was
    torch.cuda.synchronize()
    assert got.shape == (256, 256, 32) and bool(torch.isfinite(got).all())
    assert float(got[..., :31].float().std()) > 1e-2
    d = (got.float() - ref.float()).abs()
    return got, ref, float(d.mean()), float(d.max())


def test_forward_256_with_and_without_the_whole_line_upsampling():
    """One 256^2 forward pass, the default route against _AVX._convt_lines = False.  Bit-identical where no step with a Gram epilogue moved (`out` is
    the K = 16 kernel's to the bit); a moved step with the epilogue sums its Gram partials over other workgroups, and the full-resolution step moves
    from the K = 8 kernel: then two float16 evaluations of one network, held to the project's yardstick (mean <= 2.2e-4, max <= 6e-3)."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    got, ref, mean, mx = _forward_pair(lambda a: None)
    print(f"256^2 forward, default route vs AVX_MST_NO_CONVT_LINES: CONVT_LINES_C {_AVX.CONVT_LINES_C}, CONVT_LINES_GRAM_C {_AVX.CONVT_LINES_GRAM_C}: mean {mean:.3e}, max {mx:.3e}")
    if not _AVX.CONVT_LINES_GRAM_C:
        assert torch.equal(got, ref)
    else:
        assert mean <= 2.2e-4 and mx <= 6e-3, (mean, mx)


def test_forward_256_with_every_step_on_the_whole_line_form():
    """The same with both decoder steps forced onto the whole-line kernels with their epilogues, whatever the default route holds."""

    def every(a):
        a.CONVT_LINES_C, a.CONVT_LINES_GRAM_C = (64, 128), (64, 128)

    _, _, mean, mx = _forward_pair(every)
    print(f"256^2 forward, both decoder steps on the whole-line form vs none: mean {mean:.3e}, max {mx:.3e}")
    assert mean <= 2.2e-4 and mx <= 6e-3, (mean, mx)
