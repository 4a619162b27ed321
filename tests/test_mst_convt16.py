"""Host side of the K = 16 decoder upsampling (csrc/mst_mfma.hip::k_mst_convt2x2_16): the fragment orders, under the CPU lane model of
v_mfma_f32_32x32x16_f16 that tests/test_mstpp.py uses (A: lane -> row lane % 32, k = 8 * (lane // 32) + j; B likewise with columns; D: lane ->
column lane % 32, rows (v & 3) + 8 * (v >> 2) + 4 * (lane // 32))."""
import numpy as np
import torch


def _mfma16(D, a, b):
    """D (32, 32) += A B^T for one instruction: a, b are (64 lanes, 8) fragments."""
    for half in range(2):
        D += a[half * 32:(half + 1) * 32, :] @ b[half * 32:(half + 1) * 32, :].T
    return D


def test_pack_fragments16_halfrow_reproduces_the_gemm_with_a_lanes_half_row_as_the_operand():
    """The operand of step s is the s-th 16-byte load of a lane's contiguous half row (lane (pixel, h): channels h K/2 + 8 s + j), at the two
    input widths of the upsampling kernel and the widths of its skip product; every result lane must hold 16 CONTIGUOUS output channels."""
    from animal_vision_amd.ml.mst_plus_plus import pack_fragments16

    rng = np.random.default_rng(12)
    lane = np.arange(64)
    px, hh = lane % 32, lane // 32
    for K, N in ((64, 32), (128, 64), (32, 32), (64, 64)):
        x = rng.standard_normal((32, K)).astype(np.float32)
        w = rng.standard_normal((K, N)).astype(np.float32)
        want = x @ w
        frag = pack_fragments16(torch.from_numpy(w), halfrow=True).numpy()  # (N/32, K/16, 64, 8)
        assert frag.shape == (N // 32, K // 16, 64, 8)
        half_row = np.stack([x[px, hh * (K // 2) + c] for c in range(K // 2)], axis=1)  # (64 lanes, K/2): what the lane loads, in load order
        for t in range(N // 32):
            D = np.zeros((32, 32), np.float32)  # rows = (permuted) output channels, columns = pixels
            for s in range(K // 16):
                _mfma16(D, frag[t, s], half_row[:, 8 * s:8 * s + 8])
            for half in range(2):
                for v in range(16):
                    row = (v & 3) + 8 * (v >> 2) + 4 * half
                    np.testing.assert_allclose(D[row, :], want[:, 32 * t + 16 * half + v], rtol=1e-5, atol=1e-4)


def test_the_half_wave_trade_of_the_gram_epilogue_yields_the_operand_of_pack_qkv16():
    """At 64 output channels a result lane (pixel, h) holds channels 32 t + 16 h + v of tile t (eight packed words per tile).  One
    v_permlane32_swap per word (lanes 32-63 of the tile 0 register <-> lanes 0-31 of the tile 1 register) must leave lane (pixel, h) with channels
    32 h + 8 s + j in step s -- the operand order of pack_qkv16 -- so that q and k ("pixels x channels": D rows = pixels, lane = channel) come
    out as out @ W_q^T and out @ W_k^T under the lane model."""
    from animal_vision_amd.ml.mst_plus_plus import pack_qkv16

    rng = np.random.default_rng(13)
    lane = np.arange(64)
    px, hh = lane % 32, lane // 32
    c = 64
    o = rng.standard_normal((32, c)).astype(np.float32)  # 32 output pixels
    wqkv = rng.standard_normal((c, 3 * c)).astype(np.float32)
    want = o @ wqkv
    frag = pack_qkv16(torch.from_numpy(wqkv)).numpy()  # (6 tiles, 4 steps, 64, 8)
    a = np.stack([o[px, 16 * hh + v] for v in range(16)], axis=1)       # tile 0 as the lanes hold it: (64 lanes, 16 channels)
    b = np.stack([o[px, 32 + 16 * hh + v] for v in range(16)], axis=1)  # tile 1
    a2, b2 = a.copy(), b.copy()
    a2[32:], b2[:32] = b[:32], a[32:]                                   # the swap, word by word
    steps = [a2[:, :8], a2[:, 8:], b2[:, :8], b2[:, 8:]]
    for s in range(4):
        np.testing.assert_array_equal(steps[s], np.stack([o[px, 32 * hh + 8 * s + j] for j in range(8)], axis=1))
    for t in range(4):  # q heads 0, 1, then k heads 0, 1
        D = np.zeros((32, 32), np.float32)  # rows = pixels, columns = channels of the tile
        for s in range(4):
            _mfma16(D, steps[s], frag[t, s])
        np.testing.assert_allclose(D, want[:, 32 * t:32 * t + 32], rtol=1e-5, atol=1e-4)
