"""Float64 NumPy references of the training side path, written from include/nic.h.

Each function restates the formula the header gives for its entry point as a loop over taps
with array indexing -- no library convolution -- so any pad, stride, output size and either
weight layout is covered.  The dispatch rules of csrc/nic_train.hip (tile16, the vec / ph
conditions, wgrad_na, wgrad_slices) are restated as small pure functions so that the case
tables below can say which kernel form each case runs; tests/test_train_ref.py checks the
references against torch in float64 and the tables against the rules, and
tests/test_gpu_train_domain.py runs the tables on the GPU."""
from collections import namedtuple

import numpy as np


# ---- nic_conv_gather / nic_conv_gather_act ----------------------------------------------------
def _src_index(o_count, k, stride, pad, transposed, size):
    """Output positions o and their source positions along one axis for tap k:
    transposed 0: src = stride * o + k - pad; 1: src = (o + pad - k) / stride where it divides.
    Only pairs whose source lies inside [0, size) are returned (outside contributes 0)."""
    o = np.arange(o_count)
    if transposed:
        t = o + pad - k
        ok = (t >= 0) & (t % stride == 0)
        src = t // stride
    else:
        src = stride * o + k - pad
        ok = np.ones(o_count, dtype=bool)
    ok &= (src >= 0) & (src < size)
    return o[ok], src[ok]


def gather_ref(x, wt, layout, stride, pad, transposed, out_hw, cout, bias=None, act=0):
    """y[b][oy][ox][co] = bias[co] + sum over taps, ci of x[b][src_y][src_x][ci] W(ky,kx,ci,co);
    wt is (kh, kw, cin, cout) for layout 0 and (kh, kw, cout, cin) for layout 1."""
    x = np.asarray(x, dtype=np.float64)
    wt = np.asarray(wt, dtype=np.float64)
    n, h, w, cin = x.shape
    kh, kw = wt.shape[:2]
    assert wt.shape[2:] == ((cin, cout) if layout == 0 else (cout, cin))
    oh, ow = out_hw
    y = np.zeros((n, oh, ow, cout), dtype=np.float64)
    for ky in range(kh):
        oy, sy = _src_index(oh, ky, stride, pad[0], transposed, h)
        for kx in range(kw):
            ox, sx = _src_index(ow, kx, stride, pad[1], transposed, w)
            if oy.size == 0 or ox.size == 0:
                continue
            wk = wt[ky, kx] if layout == 0 else wt[ky, kx].T  # (cin, cout)
            y[:, oy[:, None], ox[None, :], :] += x[:, sy[:, None], sx[None, :], :] @ wk
    if bias is not None:
        y += np.asarray(bias, dtype=np.float64)
    if act:
        y = np.where(y > 0, y, 0.2 * y)
    return y


# ---- nic_conv_wgrad ------------------------------------------------------------------------
def wgrad_ref(gat, dirt, kh, kw, stride, pad):
    """dw[ky][kx][a][b'] = sum over b, u of gat[b][stride*uy+ky-pad_y][stride*ux+kx-pad_x][a] *
    dir[b][uy][ux][b']."""
    gat = np.asarray(gat, dtype=np.float64)
    dirt = np.asarray(dirt, dtype=np.float64)
    n, gh, gw, ca = gat.shape
    _, uh, uw, cb = dirt.shape
    dw = np.zeros((kh, kw, ca, cb), dtype=np.float64)
    for ky in range(kh):
        uy, gy = _src_index(uh, ky, stride, pad[0], 0, gh)
        for kx in range(kw):
            ux, gx = _src_index(uw, kx, stride, pad[1], 0, gw)
            if uy.size == 0 or ux.size == 0:
                continue
            g = gat[:, gy[:, None], gx[None, :], :].reshape(-1, ca)
            d = dirt[:, uy[:, None], ux[None, :], :].reshape(-1, cb)
            dw[ky, kx] = g.T @ d
    return dw


# ---- nic_act_bias_grad -----------------------------------------------------------------------
def act_bias_grad_ref(y, dy, act, dtype=np.float64):
    """dz = dy * (act && !(y > 0) ? 0.2 : 1) evaluated in `dtype` (one multiply: in float32 it is
    the kernel's dz bit for bit), db[c] = the float64 sum over rows of that dz."""
    dy = np.asarray(dy, dtype=dtype)
    dz = dy
    if act:
        dz = np.where(np.asarray(y) > 0, dy, dy * dtype(0.2)).astype(dtype)
    db = dz.reshape(-1, dz.shape[-1]).astype(np.float64).sum(axis=0)
    return dz, db


# ---- nic_gauss_1d ----------------------------------------------------------------------------
def gauss_1d_ref(t, taps, vertical, adjoint):
    """One-channel planes (n, h, w): VALID correlation out[i] = sum_k taps[k] in[i + k] along x
    (vertical 0) or y, or its adjoint out[i] = sum_k taps[k] in[i - k] (d = ntaps - 1 longer)."""
    t = np.asarray(t, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    if vertical:
        return gauss_1d_ref(t.transpose(0, 2, 1), taps, 0, adjoint).transpose(0, 2, 1)
    n, h, w = t.shape
    d = taps.size - 1
    if adjoint:
        out = np.zeros((n, h, w + d), dtype=np.float64)
        for k in range(taps.size):
            out[:, :, k:k + w] += taps[k] * t
    else:
        out = np.zeros((n, h, w - d), dtype=np.float64)
        for k in range(taps.size):
            out += taps[k] * t[:, :, k:k + w - d]
    return out


def gauss_window(size=11, sigma=1.5):
    """The normalised Gaussian of tf.image.ssim, as training._gauss_window builds it."""
    c = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = np.exp(-0.5 * c * c / sigma ** 2)
    return g / g.sum()


# ---- the lum cs mean of nic_msssim_terms / nic_msssim_terms_grad (train_hip.ssim_map_mean) -----
def _ssim_terms(mx, my, sxy, sxx, c1, c2):
    mx, my, sxy, sxx = (np.asarray(t, dtype=np.float64) for t in (mx, my, sxy, sxx))
    num0 = mx * my * 2.0
    den0 = mx * mx + my * my
    a, b = num0 + c1, den0 + c1
    c, d = 2.0 * sxy - num0 + c2, sxx - den0 + c2
    return mx, my, a, b, c, d


def ssim_map_ref(mx, my, sxy, sxx, c1, c2):
    """(n,) mean over each plane of lum cs, lum = (num0 + c1)/(den0 + c1), cs = ((2 sxy - num0) +
    c2)/((sxx - den0) + c2), num0 = 2 mx my, den0 = mx^2 + my^2.  Operands (n, ...)."""
    _, _, a, b, c, d = _ssim_terms(mx, my, sxy, sxx, c1, c2)
    v = (a / b) * (c / d)
    return v.reshape(v.shape[0], -1).mean(axis=1)


def ssim_map_grad_ref(mx, my, sxy, sxx, g, c1, c2):
    """Gradients of sum_i g[i] ssim_mean[i] with respect to mx, my, sxy, sxx (analytic)."""
    mx, my, a, b, c, d = _ssim_terms(mx, my, sxy, sxx, c1, c2)
    n = mx.shape[0]
    hw = mx.size // n
    G = (np.asarray(g, dtype=np.float64) / hw).reshape((n,) + (1,) * (mx.ndim - 1))
    lum, cs = a / b, c / d
    # d lum / d mx = (2 my b - 2 mx a) / b^2, d cs / d mx = (-2 my d + 2 mx c) / d^2; my alike
    gmx = G * (cs * (2 * my * b - 2 * mx * a) / (b * b) + lum * (-2 * my * d + 2 * mx * c) / (d * d))
    gmy = G * (cs * (2 * mx * b - 2 * my * a) / (b * b) + lum * (-2 * mx * d + 2 * my * c) / (d * d))
    gsxy = G * lum * 2.0 / d
    gsxx = -G * lum * c / (d * d)
    return gmx, gmy, gsxy, gsxx


# ---- nic_absmax_scale ------------------------------------------------------------------------
def absmax_scale_ref(x):
    """2^(13 - floor(log2 max|x|)), the exponent held to -126..126; 1 when the maximum is 0 or
    infinite.  The maximum skips NaN elements (so does fmaxf): a tensor of NaNs alone has
    maximum 0."""
    a = np.abs(np.asarray(x, dtype=np.float64).ravel())
    a = a[~np.isnan(a)]
    m = a.max() if a.size else 0.0
    if m == 0.0 or not np.isfinite(m):
        return 1.0
    _, e = np.frexp(m)  # m = f 2^e, f in [0.5, 1): floor(log2 m) = e - 1
    return float(np.ldexp(1.0, int(np.clip(13 - (e - 1), -126, 126))))


# ---- dispatch and work-size rules of csrc/nic_train.hip ------------------------------------------
def tile16(c):
    return 16 if c <= 16 else 32 if c <= 32 else 64


def gather_form(cin, cout, transposed, stride, aligned=True):
    """(NT, VEC, PH) of conv_gather_kernel as launch_conv_gather picks it."""
    vec = cin % 32 == 0 and bool(aligned)
    ph = vec and bool(transposed) and stride == 2
    return tile16(cout), vec, ph


def wgrad_form(kh, kw, ca, cb):
    """(NA, NB) of conv_wgrad_kernel as launch_conv_wgrad picks it."""
    rows = kh * kw * ca
    return (64 if rows > 32 else 32 if rows > 16 else 16), tile16(cb)


def _cdiv(a, b):
    return -(-a // b)


def gather_work_bytes(kh, kw, cin, cout):
    """chunks x co tiles x 2 (hi, lo) x 64 lanes x 16 B."""
    return _cdiv(kh * kw * cin, 32) * (tile16(cout) // 16) * 2 * 64 * 16


def wgrad_slices(n, uh, uw, kh, kw, ca, cb):
    U, rows = n * uh * uw, kh * kw * ca
    rowblocks = _cdiv(rows, wgrad_form(kh, kw, ca, cb)[0])
    return max(1, min(_cdiv(2048, rowblocks), _cdiv(U, 4 * 32)))


def wgrad_work_floats(n, uh, uw, kh, kw, ca, cb):
    """slices x rows x cb."""
    return wgrad_slices(n, uh, uw, kh, kw, ca, cb) * kh * kw * ca * cb


def act_bias_grad_work_floats(rows, cols):
    """ceil(rows / 256) x (cols + 1)."""
    return _cdiv(rows, 256) * (cols + 1)


def ssim_map_work_floats(n, hw):
    """n x ceil(hw / 1024): the blocks of nic_msssim_terms, whose work holds two partials for each."""
    return n * _cdiv(hw, 1024)


# ---- case tables: the smallest shapes that reach each path -------------------------------------
# aligned: x is 16-byte aligned (False: a view one float into a larger buffer).  form: the
# (NT, VEC, PH) the case is meant to run, checked against gather_form on the CPU.
GatherCase = namedtuple("GatherCase", "id n h w cin cout kh kw stride pad transposed layout out_hw aligned form reaches")

GATHER_CASES = [
    GatherCase("g1", 2, 7, 9, 3, 5, 3, 3, 1, (1, 1), 0, 0, (7, 9), True, (16, False, False),
               "K = 27 in one partial chunk; M = 126 (partial last block); scalar stores"),
    GatherCase("g2", 1, 11, 13, 5, 16, 5, 5, 2, (1, 2), 0, 0, (6, 7), True, (16, False, False),
               "4 chunks, every one straddling taps; unequal pads"),
    GatherCase("g3", 2, 6, 5, 32, 9, 3, 3, 1, (1, 1), 0, 1, (6, 5), True, (16, True, False), "layout 1"),
    GatherCase("g4", 2, 4, 5, 7, 20, 4, 3, 3, (2, 1), 1, 1, (11, 14), True, (32, False, False),
               "scalar transposed; kh != kw; the % stride branch"),
    GatherCase("g5", 1, 8, 8, 17, 50, 3, 3, 1, (1, 1), 0, 0, (8, 8), True, (64, False, False),
               "fourth co tile 2 of 16 filled; cout % 4 != 0"),
    GatherCase("g6", 3, 5, 7, 64, 48, 1, 1, 1, (0, 0), 0, 0, (5, 7), True, (64, True, False),
               "vector stores with an empty fourth tile; one tap"),
    GatherCase("g7", 2, 5, 6, 32, 33, 5, 3, 2, (2, 1), 1, 1, (9, 11), True, (64, True, True),
               "odd oh, ow; tap counts differ per phase"),
    GatherCase("g8", 2, 1, 3, 64, 64, 5, 5, 2, (2, 2), 1, 1, (1, 5), True, (64, True, True),
               "phase mode with oh = 1: two phases have no pixels"),
    GatherCase("g9a", 2, 5, 6, 32, 33, 5, 3, 2, (2, 1), 1, 1, (9, 11), False, (64, False, False),
               "g7 misaligned: the scalar fallback, transposed, stride 2, multi-chunk"),
    GatherCase("g9b", 2, 9, 8, 64, 64, 5, 5, 2, (1, 1), 1, 1, (18, 16), False, (64, False, False),
               "Keras dconv7 misaligned: the fallback also switches phase mode off"),
    GatherCase("g10", 1, 9, 9, 1, 1, 8, 8, 1, (3, 3), 0, 0, (8, 8), True, (16, False, False),
               "kh * kw = 64, the documented maximum"),
    GatherCase("g11", 2, 6, 6, 64, 17, 3, 3, 2, (0, 0), 1, 0, (13, 13), True, (32, True, True),
               "phase mode with a partial tile; layout 0 transposed"),
    # the two forms the Keras shapes reach (dconv8, conv8), here at edge shapes of their own
    GatherCase("g12", 2, 3, 4, 32, 3, 3, 3, 2, (1, 1), 1, 1, (5, 8), True, (16, True, True),
               "phase mode, one partly filled tile, scalar stores"),
    GatherCase("g13", 1, 5, 4, 32, 24, 2, 2, 1, (0, 1), 0, 0, (4, 4), True, (32, True, False),
               "even kernel, unequal pads, second tile half filled"),
]

WgradCase = namedtuple("WgradCase", "id n uh uw ca cb kh kw stride pad gat_hw form reaches")

WGRAD_CASES = [
    WgradCase("w1", 2, 5, 6, 1, 1, 3, 3, 1, (1, 1), (5, 6), (16, 16), "9 rows"),
    WgradCase("w2", 3, 4, 5, 3, 20, 2, 2, 1, (0, 1), (5, 5), (16, 32), "12 rows; cb tail"),
    WgradCase("w3", 2, 6, 6, 16, 64, 1, 1, 1, (0, 0), (6, 6), (16, 64), "one tap"),
    WgradCase("w4", 2, 5, 5, 3, 5, 3, 3, 2, (1, 1), (9, 10), (32, 16), "27 rows"),
    WgradCase("w5", 2, 6, 7, 20, 16, 3, 3, 1, (1, 1), (6, 7), (64, 16),
              "180 rows = 3 blocks, the last partial; row blocks span taps"),
    WgradCase("w6", 2, 4, 5, 33, 33, 5, 5, 2, (1, 2), (8, 10), (64, 64),
              "825 rows; ca does not divide 64; cb tail"),
    WgradCase("w7", 5, 2, 1, 32, 32, 3, 3, 1, (1, 1), (2, 1), (64, 32),
              "uw = 1: a 4-pixel item crosses rows and images; U = 10"),
    WgradCase("w8", 1, 1, 3, 64, 64, 3, 3, 1, (1, 1), (1, 3), (64, 64), "U = 3 < 4"),
    WgradCase("w9", 1, 25, 40, 64, 32, 4, 3, 3, (2, 0), (74, 118), (64, 32),
              "stride 3; kh != kw; U = 1000: 8 slices of 128, slice ends inside a row"),
    # the two forms the Keras shapes reach (conv1, dconv8), here at edge shapes of their own
    WgradCase("w10", 2, 3, 4, 2, 24, 3, 3, 1, (1, 1), (3, 4), (32, 32), "18 rows; cb tail"),
    WgradCase("w11", 1, 4, 4, 5, 40, 2, 2, 1, (0, 0), (5, 5), (32, 64), "20 rows; cb tail"),
]

ABG_COLS = (3, 5, 20, 50, 63, 4, 12, 60)
ABG_ROWS = (1, 255, 257, 700)
SSIM_HW = ((1, 1), (31, 33), (32, 32), (25, 41))  # hw = 1, 1023, 1024, 1025
SSIM_N = (1, 65)
