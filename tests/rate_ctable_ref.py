"""A float64 NumPy restatement of the context rate loss, the yardstick of
tests/test_rate_ctable.py and tests/test_gpu_rate_ctable.py.  Not a test.

L is (G * C, 3, 256) code lengths in bits, anchors G * C bytes; y and yc are (M, h, w, C) NHWC;
rows as tests/rate_table_ref.py.  Element (m, q, c), q the row-major pixel inside plane m:

    x = 0 if q % seg_pixels == 0, else min(2, |rint(min(max(255 yc[m][q-1][c], 0), 255)) - anchors[r]|)
    v, k, t as the table rate's,  bits = L[r][x][k] + t (L[r][x][k+1] - L[r][x][k]).

The discrete steps (the context, k) and t's operand v are taken in fp32, as rate_table_ref takes
them: an fp32 product that lands on the other side of an integer or of a half than the float64
product would is not an error of the arithmetic being measured.
"""
import numpy as np

from tests import rate_table_ref as R

# section 21's shapes and 15 planes of 16 x 16 x 32: eight forward blocks per plane, ten 128-pixel
# slabs per group in the backward, the last one ragged
SHAPES = R.SHAPES + [(15, 16, 16, 32, 3)]  # (M, h, w, C, G)


def segs(shape):
    """seg_pixels of a shape: everything in context 0; segments that end mid-row and slabs that begin
    mid-segment; the container's default; only q = 0 in context 0."""
    return [1, 5, 32, shape[1] * shape[2] + 1]


def code_lengths(logits):
    """-log2(softmax(logits, axis=-1)) in float64."""
    z = np.asarray(logits, np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    return -(z - np.log(np.exp(z).sum(axis=-1, keepdims=True))) / np.log(2.0)


def codes_of(yc):
    """rint(min(max(255 yc, 0), 255)) with the fp32 product; int64."""
    yc = np.asarray(yc, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.float32(255.0) * yc
    v = np.fmin(np.fmax(v, np.float32(0)), np.float32(255))  # fmax / fmin drop a NaN
    return np.rint(v).astype(np.int64)  # to nearest, ties to even


def contexts(yc, anchors, groups, seg_pixels):
    """(M, h, w, C) contexts in 0..2."""
    m, h, w, c = yc.shape
    code = codes_of(yc).reshape(m, h * w, c)
    a = np.asarray(anchors, np.int64)[R.rows_of(m, c, groups).reshape(m, 1, c)]
    ctx = np.zeros_like(code)
    ctx[:, 1:] = np.minimum(2, np.abs(code[:, :-1] - a))
    ctx[:, ::seg_pixels] = 0
    return ctx.reshape(m, h, w, c)


def rate_ctable(y, L, anchors, groups, seg_pixels, yc=None):
    """-> (plane_bits (M,), abs_sum (M,)): the sums and the sums of the absolute terms."""
    L = np.asarray(L, np.float64)
    m, _, _, c = y.shape
    k, t = R.elements(y)
    x = contexts(y if yc is None else yc, anchors, groups, seg_pixels)
    r = R.rows_of(m, c, groups)
    l0, l1 = L[r, x, k], L[r, x, k + 1]
    bits = l0 + t * (l1 - l0)
    return bits.sum(axis=(1, 2, 3)), (np.abs(l0) + np.abs(t * (l1 - l0))).sum(axis=(1, 2, 3))


def rate_ctable_grad(y, L, anchors, g, groups, seg_pixels, yc=None, autograd_terms=False):
    """-> (dy (M, h, w, C), dL (G C, 3, 256), dL_abs): as rate_table_ref.rate_table_grad."""
    L = np.asarray(L, np.float64)
    g = np.asarray(g, np.float64)
    m, _, _, c = y.shape
    k, t = R.elements(y)
    x = contexts(y if yc is None else yc, anchors, groups, seg_pixels)
    r = np.broadcast_to(R.rows_of(m, c, groups), k.shape)
    gm = np.broadcast_to(g[:, None, None, None], k.shape)
    dy = 255.0 * gm * (L[r, x, k + 1] - L[r, x, k])
    dL, dL_abs = np.zeros_like(L), np.zeros_like(L)
    for acc, wt in ((dL, gm), (dL_abs, np.abs(gm))):
        np.add.at(acc, (r, x, k), wt * (1.0 + t) if autograd_terms and acc is dL_abs else wt * (1.0 - t))
        np.add.at(acc, (r, x, k + 1), wt * t)
    return dy, dL, dL_abs


def case(shape, seed=0):
    """Inputs of one shape: y (the noisy latent), yc (the clean one the contexts are read from), both
    (M, h, w, C) fp32 in [0, 1], anchors (G C,) u8 and logits (G C, 3, 256) fp32.  A channel's codes
    are an AR(1) walk around its anchor, so neighbours are correlated, the anchors lie near the data
    and the three contexts all occur; y holds some exact codes, zeros and ones."""
    m, h, w, c, groups = shape
    rng = np.random.default_rng(seed + 1000 * m + 10 * h + w)
    anchors = rng.integers(2, 254, groups * c).astype(np.uint8)
    a = anchors.astype(np.float64)[R.rows_of(m, c, groups).reshape(m, c)]
    d = np.zeros((m, h * w, c))
    prev = np.zeros((m, c))
    for q in range(h * w):
        prev = np.rint(0.5 * prev + 1.2 * rng.standard_normal((m, c)))
        d[:, q] = prev
    code = np.clip(a[:, None, :] + d, 0, 255).reshape(m, h, w, c)
    yc = ((code + rng.uniform(-0.3, 0.3, code.shape)) / 255.0).clip(0, 1).astype(np.float32)
    y = ((code + rng.uniform(-0.5, 0.5, code.shape)) / 255.0).clip(0, 1).astype(np.float32)
    pick = rng.random(y.shape)
    y[pick < 0.05] = 0.0
    y[pick > 0.95] = 1.0
    exact = (code / np.float32(255)).astype(np.float32)
    y = np.where((pick > 0.4) & (pick < 0.55), exact, y)
    yc = np.where((pick > 0.5) & (pick < 0.7), exact, yc)
    logits = (2.0 * rng.standard_normal((groups * c, 3, 256))).astype(np.float32)
    return y, yc, anchors, logits


def assert_contexts_occur(shape):
    """At a shape with at least 9 pixels all three contexts occur in every group (for every
    seg_pixels but 1, where everything is context 0)."""
    m, h, w, c, groups = shape
    y, yc, anchors, _ = case(shape)
    for seg in segs(shape)[1:]:
        for src in (y, yc):
            x = contexts(src, anchors, groups, seg).reshape(groups, -1)
            for grp in range(groups):
                assert set(np.unique(x[grp])) == {0, 1, 2}, (shape, seg, grp)


def edge_case(c=32, groups=3):
    """Section 21's edge values in y and in yc: every exact code, the float just below it, the
    half-way points (k + 0.5) / 255 (the ties of rint), -0.5, 1.5, NaN, 0, 1 and both infinities,
    and the clamped tensors that must give the same results.  -> (y, yc, y_clamped, yc_clamped,
    anchors), the tensors (3, n, 16, c)."""
    f = np.float32
    codes = (np.arange(256) / f(255)).astype(f)
    halves = ((np.arange(255) + f(0.5)) / f(255)).astype(f)
    vals = np.concatenate([codes, np.nextafter(codes, f(-1)), halves,
                           f([-0.5, 1.5, np.nan, 0.0, 1.0, np.inf, -np.inf])])
    n = -(-vals.size // 16)
    flat = np.resize(vals, n * 16)
    y = np.broadcast_to(flat.reshape(1, n, 16, 1), (3, n, 16, c)).copy()
    yc = np.roll(y, 7, axis=1)[:, :, ::-1].copy()  # the same values at other places
    rng = np.random.default_rng(7)
    anchors = rng.integers(0, 256, groups * c).astype(np.uint8)

    def clamp(t):
        with np.errstate(invalid="ignore"):
            return np.where(np.isnan(t), f(0), np.clip(t, 0, 1)).astype(f)

    return y, yc, clamp(y), clamp(yc), anchors


def planes_of(z):
    """u8 latents (N, h, w, 96) -> (y (3 N, h, w, 32) fp32 = z / 255, the planes of group g being
    channels 32 g .. 32 g + 31 of the N images in order)."""
    z = np.asarray(z)
    n, h, w, ch = z.shape
    p = z.reshape(n, h, w, 3, ch // 3).transpose(3, 0, 1, 2, 4).reshape(3 * n, h, w, ch // 3)
    return (p / np.float32(255)).astype(np.float32)
