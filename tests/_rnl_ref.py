"""The yardstick of the receptor-noise-limited colour distance (Vorobyev & Osorio 1998) in NumPy float64 -- the
definition of include/avx.h above avx_receptor_delta_u8, no code under test.

The observer: a K x 3 matrix R on linear RGB (K = 2, 3 or 4), the Weber fraction e_i of every class, and the floor eps.  Every row of R
is divided by its own sum in float64 (R'; rounded to float32 once where dtype is float32).  The catch of a pixel: with lin the decode
table of _deltae_ref and (r, g, b) = lin of the codes, q_i = (g + R'_i0 (r - g)) + R'_i2 (b - g): a grey has q_i = g exactly.  The
contrast: df_i = log((q_iA + eps) / (q_iB + eps)).  The distance:
  K = 2: dS = |df_1 - df_2| / sqrt(e_1^2 + e_2^2);
  K = 3, 4: dS^2 = sum over the pairs (i, j) of w_ij (df_i - df_j)^2 / D, where w_ij is the product of e_k^2 over the classes k outside
  the pair and D the sum, over the classes, of the product of e_k^2 over the other classes -- the forms written out in include/avx.h,
  the pairs in that order.
Two pixels of equal codes are 0 by definition.

dtype=np.float32 restates the same operations as a float32 device forms them: the table, R', the weights and the reciprocal of the
denominator (K = 2: of its root) are formed in float64 and rounded once, and every operation on pixels is rounded to float32."""
import numpy as np

from _deltae_ref import decode_table

# the pairs (i, j), zero-based, in the order of the numerators in include/avx.h
PAIRS = {2: [(0, 1)], 3: [(2, 1), (2, 0), (1, 0)], 4: [(3, 2), (3, 1), (2, 1), (3, 0), (2, 0), (1, 0)]}


def weights(weber):
    """(w of every pair in PAIRS' order, the denominator D), float64."""
    e2 = [float(e) * float(e) for e in weber]
    K = len(e2)
    w = [float(np.prod([e2[k] for k in range(K) if k not in pair])) for pair in PAIRS[K]]
    den = 0.0
    for out in range(K - 1, -1, -1):
        den += float(np.prod([e2[k] for k in range(K) if k != out]))
    return w, den


def delta_s_from_catches(qa, qb, weber, floor, dtype=np.float64):
    """qa, qb: catches (..., K) of the two pixels -> dS (...)."""
    qa, qb = np.asarray(qa, dtype), np.asarray(qb, dtype)
    K = qa.shape[-1]
    assert qb.shape == qa.shape and K == len(weber) and K in PAIRS
    eps = dtype(floor)
    df = np.log((qa + eps) / (qb + eps))
    w, den = weights(weber)
    if K == 2:
        out = np.abs(df[..., 0] - df[..., 1]) / np.sqrt(den) if dtype is np.float64 else np.abs(df[..., 0] - df[..., 1]) * dtype(1.0 / np.sqrt(den))
    else:
        num = None
        for (i, j), wij in zip(PAIRS[K], w):
            d = df[..., i] - df[..., j]
            t = dtype(wij) * (d * d)
            num = t if num is None else num + t
        out = np.sqrt(num / den) if dtype is np.float64 else np.sqrt(num * dtype(1.0 / den))
    assert out.dtype == dtype
    return out


def catches(rgb8, matrix, dtype=np.float64):
    """uint8 (..., 3) -> the catches (..., K) under the row-normalised matrix, in the anchored form."""
    m = np.asarray(matrix, np.float64)
    m = (m / m.sum(axis=1, keepdims=True)).astype(dtype)
    lin = decode_table().astype(dtype)[np.asarray(rgb8)]
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    dr, db = r - g, b - g
    q = np.stack([(g + m[i, 0] * dr) + m[i, 2] * db for i in range(len(m))], axis=-1)
    assert q.dtype == dtype
    return q


def delta_s(a, b, matrix, weber, floor, dtype=np.float64):
    """uint8 (..., 3) pairs -> dS (...); exactly 0 where the codes are equal."""
    a, b = np.asarray(a), np.asarray(b)
    ds = delta_s_from_catches(catches(a, matrix, dtype), catches(b, matrix, dtype), weber, floor, dtype)
    return np.where((a == b).all(axis=-1), dtype(0.0), ds)
