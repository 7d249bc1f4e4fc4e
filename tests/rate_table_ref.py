"""A float64 NumPy restatement of the table rate loss, the yardstick of
tests/test_rate_table.py and tests/test_gpu_rate_table.py.  Not a test.

L is (G * C, 256) code lengths in bits; y is (M, h, w, C) NHWC; plane m belongs to group
m // (M / G) and its channel c reads row r = group * C + c.  Per element

    v = min(max(255 y, 0), 255)  (a NaN becomes 0),  k = min(floor(v), 254),  t = v - k,
    bits = L[r][k] + t (L[r][k+1] - L[r][k]).

The element step (v, k, t) is taken in fp32, as the code under test takes it: k is a discrete
choice and an fp32 product 255 y that lands on the other side of an integer than the float64
product would is not an error of the arithmetic being measured; v and t are then exact in float64.
"""
import numpy as np

SHAPES = [(3, 1, 1, 32, 3), (6, 5, 7, 32, 3), (2, 3, 3, 32, 1), (4, 2, 2, 8, 2),  # (M, h, w, C, G)
          # the dL kernel's replica count R = 64 // C at its ends: R = 1 (no replica sum), 64 % C != 0
          # (16 idle lanes), and R = 64 with C x 256 = 256 (the whole LDS array in use)
          (2, 3, 3, 64, 1), (2, 3, 3, 24, 2), (2, 3, 3, 1, 1)]


def code_lengths(logits):
    """-log2(softmax(logits, axis=1)) in float64."""
    z = np.asarray(logits, np.float64)
    z = z - z.max(axis=1, keepdims=True)
    return -(z - np.log(np.exp(z).sum(axis=1, keepdims=True))) / np.log(2.0)


def elements(y):
    """(k, t) of every element: k int64, t float64, from the fp32 element step."""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.float32(255.0) * y
    v = np.fmin(np.fmax(v, np.float32(0)), np.float32(255))  # fmax / fmin drop a NaN
    k = np.minimum(np.floor(v).astype(np.int64), 254)
    return k, v.astype(np.float64) - k


def rows_of(m, c, groups):
    """(M, 1, 1, C) row index of every plane and channel."""
    group = np.arange(m) // max(m // groups, 1)
    return (group[:, None] * c + np.arange(c)[None, :])[:, None, None, :]


def rate_table(y, L, groups):
    """-> (plane_bits (M,), abs_sum (M,)): the sums and the sums of the absolute terms."""
    L = np.asarray(L, np.float64)
    m, _, _, c = y.shape
    k, t = elements(y)
    r = rows_of(m, c, groups)
    l0, l1 = L[r, k], L[r, k + 1]
    bits = l0 + t * (l1 - l0)
    return bits.sum(axis=(1, 2, 3)), (np.abs(l0) + np.abs(t * (l1 - l0))).sum(axis=(1, 2, 3))


def rate_table_grad(y, L, g, groups, autograd_terms=False):
    """-> (dy (M, h, w, C), dL (G C, 256), dL_abs): the gradients of sum_m g[m] plane_bits[m], and
    the sum of the absolute terms of every entry of dL: |g| (1 - t) at k and |g| t at k + 1, or with
    ``autograd_terms`` |g| + |g| t at k, the two terms g and -g t that autograd through
    L[k] + t (L[k+1] - L[k]) adds there."""
    L = np.asarray(L, np.float64)
    g = np.asarray(g, np.float64)
    m, _, _, c = y.shape
    k, t = elements(y)
    r = np.broadcast_to(rows_of(m, c, groups), k.shape)
    gm = np.broadcast_to(g[:, None, None, None], k.shape)
    dy = 255.0 * gm * (L[r, k + 1] - L[r, k])
    dL, dL_abs = np.zeros_like(L), np.zeros_like(L)
    for acc, w in ((dL, gm), (dL_abs, np.abs(gm))):
        np.add.at(acc, (r, k), w * (1.0 + t) if autograd_terms and acc is dL_abs else w * (1.0 - t))
        np.add.at(acc, (r, k + 1), w * t)
    return dy, dL, dL_abs


def case(shape, seed=0, edges=True):
    """Inputs of one shape: y (M, h, w, C) fp32 in [0, 1] with some exact 0, 1 and code values when
    ``edges``, logits (G C, 256) fp32."""
    m, h, w, c, groups = shape
    rng = np.random.default_rng(seed + 1000 * m + 10 * h + w)
    y = rng.random((m, h, w, c), dtype=np.float32)
    if edges:
        pick = rng.random(y.shape)
        y[pick < 0.15] = 0.0
        y[pick > 0.9] = 1.0
        codes = (rng.integers(0, 256, y.shape) / np.float32(255)).astype(np.float32)
        y = np.where((pick > 0.4) & (pick < 0.5), codes, y)
    logits = (2.0 * rng.standard_normal((groups * c, 256))).astype(np.float32)
    return y, logits


def logits_grad(logits, dL, dL_abs):
    """The gradient of the table's logits from dL through L = -log2 softmax:
    dz[r][i] = -(dL[r][i] - p[r][i] sum_j dL[r][j]) / ln 2, and the sum of its absolute terms."""
    p = np.exp(-code_lengths(logits) * np.log(2.0))
    dz = -(dL - p * dL.sum(axis=1, keepdims=True)) / np.log(2.0)
    return dz, (dL_abs + p * dL_abs.sum(axis=1, keepdims=True)) / np.log(2.0)
