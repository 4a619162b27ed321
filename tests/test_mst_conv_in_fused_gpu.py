"""conv_in recomputed from the uint8 frame in its three consumers (csrc/mst_fused.hip::k_mst_conv3x3_lds<CINR / CINX>): body.0's embedding
conv takes the frame as its input, body.0's mapping conv and conv_out take it as their residual, and conv_in's output is never stored.

The new kernels evaluate conv_in with the operands, the instructions and the order of k_mst_conv_in_u8_mfma, and keep the launch geometry and the tile
order of the kernels they stand in for, so every comparison here is BIT EQUALITY with the two-kernel route (avx_mst_conv_in_u8, then the existing entry
point): outputs, Gram matrix and column norms, catch planes and the raw per-workgroup records."""
import numpy as np
import pytest
import torch

# (H, W) of the frame, the stride it is padded to
CASES = [
    ((9, 11), 16),     # -> 16 x 16: one tile, all four borders padded
    ((37, 45), 16),    # -> 48 x 48
    ((17, 130), 16),   # -> 32 x 144: a reflection nearly as large as the frame
    ((64, 64), 16),    # no padding
    ((40, 72), 8),     # 40 rows: partial tiles
    ((464, 480), 16),  # 870 tiles, more than either grid cap: the persistent loop and the prefetch
]


@pytest.fixture(scope="module")
def pred():
    from animal_vision_amd.ml import MSTPlusPlusPredictor

    return MSTPlusPlusPredictor(None, seed=0, half=True)


@pytest.fixture(scope="module")
def weights(pred):
    """The 27 x 32 conv_in table, the three convs' fragments, the first block's q / k fragments and the honeybee's spectral weights."""
    from animal_vision_amd.animals import HoneyBee
    from animal_vision_amd.ml.mst_plus_plus import PAD, pack_qkv16

    m = pred.model
    w27 = m._w("conv_in.weight", (0,)).permute(2, 3, 1, 0).reshape(27, PAD).float().contiguous()
    a0 = "body.0.encoder_layers.0.0.blocks.0.0"
    wqkv = torch.cat([m._w(a0 + ".to_q.weight", (0, 1)), m._w(a0 + ".to_k.weight", (0, 1)), m._w(a0 + ".to_v.weight", (0, 1))], 0).t().contiguous()
    return {"w27": w27, "emb": m._frag9k16("body.0.embedding.weight"), "map": m._frag9k16("body.0.mapping.weight"), "out": m._frag9k16("conv_out.weight"),
            "wqk": pack_qkv16(wqkv), "spec": HoneyBee()._operator().padded_clone(32).weights}


@pytest.fixture(scope="module")
def operands(pred, weights):
    """(hw, stride) -> (src, conv_in's stored output, a random residual-kernel input with channel 31 zero): formed once per case and left unchanged."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    from animal_vision_amd.ml.predict import pad_amounts

    cache = {}

    def get(hw, stride):
        if (hw, stride) not in cache:
            H, W = hw
            g = torch.Generator().manual_seed(1000 * H + W)
            frame = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(pred.device)
            pads = tuple(pad_amounts(H, W, stride))
            x0 = _AVX.conv_in_u8(frame, pads, weights["w27"])
            x = torch.randn(tuple(x0.shape), generator=g).half()
            x[..., 31] = 0
            cache[(hw, stride)] = ((frame, pads, weights["w27"]), x0, x.to(pred.device).contiguous())
        return cache[(hw, stride)]

    return get


def _records_equal(pa, na, pb, nb):
    return na == nb and torch.equal(pa[:na].contiguous().view(torch.int64), pb[:nb].contiguous().view(torch.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("hw,stride", CASES)
def test_embedding_from_the_frame_equals_conv_in_then_the_gram_conv(operands, weights, hw, stride):
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    src, x0, _ = operands(hw, stride)
    want = _AVX.conv3x3_lds_gram(x0, weights["emb"], None, weights["wqk"])
    got = _AVX.conv3x3_lds_gram_cin(src, weights["emb"], weights["wqk"])
    assert got[0].shape == x0.shape
    for name, a, b in zip(("out", "gram", "nq", "nk"), got, want):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert float(got[0].float().std()) > 0 and float(got[1].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("hw,stride", CASES)
def test_residual_from_the_frame_equals_conv_in_then_the_conv(operands, weights, hw, stride):
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    src, x0, x = operands(hw, stride)
    want = _AVX.conv3x3_lds(x, weights["map"], x0)
    got = _AVX.conv3x3_lds_cin(x, weights["map"], src)
    assert torch.equal(got, want), int((got != want).sum())
    assert not torch.equal(got, _AVX.conv3x3_lds(x, weights["map"], None))  # the residual took part


@pytest.mark.gpu
@pytest.mark.parametrize("hw,stride", CASES)
def test_spectral_residual_from_the_frame_equals_conv_in_then_the_spectral_conv(operands, weights, hw, stride):
    """The crop is the unpadded frame."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX

    src, x0, x = operands(hw, stride)
    crop = (src[1][0], src[1][2], hw[0], hw[1])
    planes, partials, n = _AVX.conv3x3_lds_spectral(x, weights["out"], x0, weights["spec"], crop)
    gplanes, gpartials, gn = _AVX.conv3x3_lds_spectral_cin(x, weights["out"], src, weights["spec"], crop)
    assert gplanes.shape == (3, hw[0], hw[1])
    assert torch.equal(gplanes.view(torch.int32), planes.view(torch.int32)), int((gplanes != planes).sum())
    assert n > 0 and _records_equal(gpartials, gn, partials, n)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(72, 88), (250, 330)])
def test_forward_from_u8_is_bit_identical_with_the_route_on_and_off(pred, weights, monkeypatch, hw):
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    from animal_vision_amd.ml.predict import pad_amounts
    from animal_vision_amd.synthetic import structured_frame

    assert pred.model.can_fuse_conv_in_consumers() and pred.model.can_fuse_spectral()
    frame = torch.from_numpy(structured_frame(3 + hw[0], hw[0], hw[1])).to(pred.device)
    pads = pad_amounts(hw[0], hw[1], pred.stride)
    calls = []
    real = _AVX.conv_in_u8
    monkeypatch.setattr(_AVX, "conv_in_u8", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    cube = pred.model.forward_from_u8(frame, pads)
    planes, partials, n = pred.model.forward_from_u8(frame, pads, spectral=weights["spec"])
    assert calls == []  # conv_in's output was not materialised
    monkeypatch.setattr(_AVX, "_cinfuse", False)
    assert not pred.model.can_fuse_conv_in_consumers()
    cube0 = pred.model.forward_from_u8(frame, pads)
    planes0, partials0, n0 = pred.model.forward_from_u8(frame, pads, spectral=weights["spec"])
    assert len(calls) == 2
    assert torch.equal(cube, cube0), int((cube != cube0).sum())
    assert torch.equal(planes.view(torch.int32), planes0.view(torch.int32)) and _records_equal(partials, n, partials0, n0)


@pytest.mark.gpu
def test_honeybee_frame_is_byte_identical_with_the_route_on_and_off(pred, monkeypatch):
    from animal_vision_amd.animals import HoneyBee
    from animal_vision_amd.ml.mst_plus_plus import _AVX
    from animal_vision_amd.synthetic import structured_frame

    frame = structured_frame(75, 72, 88)
    op = HoneyBee()._operator()
    assert op.takes_catches()
    on = pred.honeybee(frame, op)
    monkeypatch.setattr(_AVX, "_cinfuse", False)
    off = pred.honeybee(frame, op)
    assert on.shape == frame.shape and np.array_equal(on, off)


def test_byte_model_falls_by_250_bytes_per_pixel(monkeypatch):
    """Four 64-byte trips of conv_in's output and conv_in's own 3-byte read of the frame go; three 3-byte reads of the frame come."""
    from animal_vision_amd.ml.mst_plus_plus import _AVX, hbm_bytes_per_px

    monkeypatch.setattr(_AVX, "_cinfuse", True)
    on = hbm_bytes_per_px()
    monkeypatch.setattr(_AVX, "_cinfuse", False)
    assert hbm_bytes_per_px() - on == 250.0
