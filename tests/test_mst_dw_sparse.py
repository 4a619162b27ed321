"""No GPU: ml/mst_plus_plus.py::pack_dw_smfmac against a NumPy lane model of v_smfmac_f32_16x16x64_f16 and v_mfma_f32_16x16x32_f16.

The model is the operand layout the one-hot probe measured on gfx950 (tools/experiments/smfmac_dw_probe.hip,
profiles/r06/probe_smfmac_dw.txt; cbsz = abid = 0):
  * D, lane l, register r: row m = 4 (l // 16) + r, column n = l % 16 (as the dense 16x16 instructions);
  * A, lane La = m + 16 qa, element e, with t = bits 2 e, 2 e + 1 of the LOW 16 bits of lane La's index register, multiplies
    B, lane n + 16 qb, element j, where qb = 2 (qa % 2) + e // 4 and j = 8 (qa // 2) + 4 ((e % 4) // 2) + t;
  * the dense instruction: A lane m + 16 q, element j multiplies B lane n + 16 q, element j.
Under it the two-instruction unit (dense shift 2, then sparse shifts 0 and 1) must reproduce a depthwise 3x3 conv exactly: the data are
multiples of 1 / 64 in float16, so every product and every sum is exact in float64."""
import numpy as np
import pytest
import torch


def smfmac_16x16x64(a, idx, b):
    """a (64, 8), idx (64,) int, b (64, 16) -> d (64, 4), float64."""
    d = np.zeros((64, 4))
    n = np.arange(16)
    for la in range(64):
        m, qa = la % 16, la // 16
        for e in range(8):
            t = (int(idx[la]) >> (2 * e)) & 3
            qb, j = 2 * (qa % 2) + e // 4, 8 * (qa // 2) + 4 * ((e % 4) // 2) + t
            d[16 * (m // 4) + n, m % 4] += a[la, e] * b[n + 16 * qb, j]
    return d


def mfma_16x16x32(a, b):
    """a (64, 8), b (64, 8) -> d (64, 4), float64."""
    d = np.zeros((64, 4))
    n = np.arange(16)
    for la in range(64):
        m, q = la % 16, la // 16
        d[16 * (m // 4) + n, m % 4] += (a[la][None, :] * b[n + 16 * q]).sum(axis=1)
    return d


def _weights(ch, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-128, 129, (ch, 1, 3, 3), generator=g).double() / 64
    w[torch.rand((ch, 1, 3, 3), generator=g) < 0.25] = 0.0  # zero taps: a pair of the compressed operand may hold two zeros
    w[0] = 0.0                                              # and a channel without any weight
    return w.half()


@pytest.mark.parametrize("ch", [8, 32, 64, 128])
def test_pack_dw_smfmac_is_the_depthwise_conv_under_the_lane_model(ch):
    from animal_vision_amd.ml.mst_plus_plus import pack_dw_mfma, pack_dw_smfmac

    w = _weights(ch, ch)
    pk = pack_dw_smfmac(w)
    assert pk.shape == (ch // 8, 3, 64, 8) and pk.dtype == torch.float16
    assert torch.equal(pk[:, 1], pack_dw_mfma(w)[:, 2])
    bits = pk.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    assert not bits[:, 2, :, 1:].any()  # the index word is 16 bits wide
    idx = bits[:, 2, :, 0]
    a_sp, a_d = pk[:, 0].double().numpy(), pk[:, 1].double().numpy()
    # 2:4 by construction: at most one non-zero per pair, and the two indices of a pair differ
    assert ((a_sp.reshape(ch // 8, 64, 4, 2) != 0).sum(axis=3) <= 1).all()
    f = np.stack([(idx >> (2 * e)) & 3 for e in range(8)], axis=2).reshape(ch // 8, 64, 4, 2)
    assert (f[..., 0] != f[..., 1]).all()
    rng = np.random.default_rng(ch)
    x = rng.integers(-128, 129, size=(4, 18, ch)).astype(np.float64) / 64  # four input rows, 16 + 2 columns
    assert (x.astype(np.float16) == x).all()
    wn = w.double().numpy()[:, 0]  # [ch][dy][dx]
    lane = np.arange(64)
    n, q = lane % 16, lane // 16
    for o in range(ch // 8):
        sh = [x[q, n + i, 8 * o:8 * o + 8] for i in range(3)]  # the unit's three 16-byte reads: lane (n, q) = row q, column n + i
        d = mfma_16x16x32(a_d[o], sh[2]) + smfmac_16x16x64(a_sp[o], idx[o], np.concatenate([sh[0], sh[1]], axis=1))
        for s in range(2):
            for c in range(8):
                m = 8 * s + c
                want = sum(wn[8 * o + c, dy, dx] * x[s + dy, np.arange(16) + dx, 8 * o + c] for dy in range(3) for dx in range(3))
                got = d[16 * (m // 4) + np.arange(16), m % 4]
                assert np.array_equal(got, want), (o, s, c)


def test_lane_models_agree_on_a_dense_operand():
    """The sparse model with both halves of every group of four spelled out (indices (0, 1) then (2, 3) in two calls) is the dense product over K = 64."""
    rng = np.random.default_rng(5)
    a = rng.integers(-8, 9, size=(16, 64)).astype(np.float64)  # [m][k], K order of the sparse instruction: lane group qa holds k = 16 qa ... + 15
    b = rng.integers(-8, 9, size=(64, 16)).astype(np.float64)  # [k][n]
    bl = np.zeros((64, 16))
    for qb in range(4):
        for j in range(16):
            bl[np.arange(16) + 16 * qb, j] = b[8 * qb + (j % 8) + 32 * (j // 8)]
    d = np.zeros((64, 4))
    for half, word in ((0, 0x4444), (1, 0xEEEE)):
        al = np.zeros((64, 8))
        for la in range(64):
            for e in range(8):
                al[la, e] = a[la % 16, 16 * (la // 16) + 4 * (e // 2) + 2 * half + e % 2]
        d += smfmac_16x16x64(al, np.full(64, word), bl)
    want = a @ b
    for m in range(16):
        assert np.array_equal(d[16 * (m // 4) + np.arange(16), m % 4], want[m])
