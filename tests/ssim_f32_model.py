"""NumPy restatement of the arithmetic of csrc/nic_quality.hip's MS-SSIM kernels.

It documents what ``ssim_tile_kernel`` and ``ssim_pool_kernel`` round and in which order, so
that a change of the arithmetic can be tried on the CPU first.  It is NOT the reference: the
GPU tests compare with the float64 oracle (``oracle.nic_oracle.ms_ssim_terms``) only.

Per scale and per (32x32 output tile, plane), as the kernel does it:
  * the 42x42 input window of both images is staged as fp32, ``u8 * (1/255)`` at scale 0,
    minus a shift, and 0 outside the image;
  * horizontal 11-tap pass over (x, y, x^2 + y^2, x*y), then the vertical pass, each a chain
    of fp32 FMAs from tap 0 to tap 10 starting at 0;
  * ``lum`` from the means with the shift added back, ``cs`` from the shifted moments; every
    elementwise operation rounded on its own (the library is built with -ffp-contract=off);
  * each thread sums its 4 outputs in fp32, a wave sums its 64 threads as a butterfly in fp32,
    the 4 wave sums of a tile and all tile sums add in fp64.
Between scales a 2x2 average pool in fp32, odd sizes repeating the last row / column.

The shift is the parameter:
  ``"fixed"``        0.5 for both images (the kernel before the local shift);
  ``"window_mean"``  per image, the fp32 mean of the in-image pixels of the tile's window
                     (the kernel now).
Covariances do not depend on the shift; what depends on it is how many fp32 bits are left
when ``E[x^2 + y^2] - (E[x]^2 + E[y]^2)`` cancels.

Two departures from the device remain: an FMA is emulated as the float64 product-and-sum
rounded to fp32 (a double rounding, off by one fp32 ulp in rare ties), and ``v_rcp_f32``
(1 ulp) is taken as the correctly rounded reciprocal.
"""
import numpy as np

F32 = np.float32
TILE, TAPS = 32, 11
WIN = TILE + TAPS - 1
SCALES = 5
SHIFTS = ("fixed", "window_mean")


def _gauss():
    d = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2.0
    g = np.exp(-0.5 * d * d / (1.5 * 1.5))
    return (g / g.sum()).astype(F32)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _butterfly(v):
    """Sum of the last axis (64 lanes) as ``v += shfl_xor(v, o)`` for o = 32 .. 1 leaves it."""
    n = v.shape[-1]
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def _lane_sum(v):
    """fp32 block sum of a (P, WIN, WIN) window as the kernel reduces it: element i belongs to
    thread i % 256, a thread adds its elements in order, a wave is a butterfly, and the four
    wave sums add left to right."""
    flat = v.reshape(v.shape[0], -1)
    pad = (-flat.shape[1]) % 256
    flat = np.concatenate([flat, np.zeros((flat.shape[0], pad), F32)], axis=1).reshape(v.shape[0], -1, 256)
    t = np.zeros((v.shape[0], 256), F32)
    for k in range(flat.shape[1]):
        t = t + flat[:, k]
    w = _butterfly(t.reshape(-1, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _filter(v, g, axis):
    n = v.shape[axis] - TAPS + 1
    acc = np.zeros_like(np.take(v, range(n), axis=axis))
    for j in range(TAPS):
        acc = _fma(g[j], np.take(v, range(j, j + n), axis=axis), acc)
    return acc


def _tile_sums(wx, wy, inside, oh, ow, shift):
    """(sum lum*cs, sum cs) in float64 over the oh x ow valid outputs of one tile, for P planes.
    wx, wy: (P, WIN, WIN) fp32 unshifted windows (anything outside); inside: (WIN, WIN) bool."""
    g = _gauss()
    half = F32(0.5)
    if shift == "fixed":
        sx = sy = np.full((wx.shape[0], 1, 1), half, F32)
    elif shift == "window_mean":
        inv = F32(1.0) / F32(inside.sum())
        sx = (_lane_sum(np.where(inside, wx, F32(0))) * inv)[:, None, None]
        sy = (_lane_sum(np.where(inside, wy, F32(0))) * inv)[:, None, None]
    else:
        raise ValueError(f"shift must be one of {SHIFTS}")
    vx = np.where(inside, wx - sx, F32(0))
    vy = np.where(inside, wy - sy, F32(0))
    maps = (vx, vy, _fma(vx, vx, vy * vy), vx * vy)
    m0, m1, e2, e3 = (_filter(_filter(m, g, 2), g, 1) for m in maps)
    c1, c2 = F32(0.01) * F32(0.01), F32(0.03) * F32(0.03)
    two, one = F32(2), F32(1)
    mx, my = m0 + sx, m1 + sy
    lum = (two * mx * my + c1) * (one / (mx * mx + my * my + c1))
    cs = (two * (e3 - m0 * m1) + c2) * (one / (e2 - (m0 * m0 + m1 * m1) + c2))
    valid = (np.arange(TILE)[:, None] < oh) & (np.arange(TILE)[None, :] < ow)
    out = []
    for q in (lum * cs, cs):
        q = np.where(valid, q, F32(0)).reshape(-1, TILE // 4, 4, TILE)  # thread (r0/4, c): rows r0..r0+3
        t = np.zeros((q.shape[0], TILE // 4, TILE), F32)
        for o in range(4):
            t = t + q[:, :, o]
        w = _butterfly(t.reshape(-1, 4, 64))  # wave w: threads 64w..64w+63 = row groups 2w, 2w+1
        out.append(w.astype(np.float64).sum(axis=1))
    return out


def _scale_terms(x, y, shift):
    """x, y: (P, H, W) fp32 -> (P, 2) float64 means of lum*cs and cs over the VALID outputs."""
    P, H, W = x.shape
    OH, OW = H - TAPS + 1, W - TAPS + 1
    px = np.zeros((P, H + WIN, W + WIN), F32)
    py = np.zeros_like(px)
    px[:, :H, :W], py[:, :H, :W] = x, y
    acc = np.zeros((P, 2))
    for y0 in range(0, OH, TILE):
        for x0 in range(0, OW, TILE):
            inside = (np.arange(y0, y0 + WIN)[:, None] < H) & (np.arange(x0, x0 + WIN)[None, :] < W)
            s, c = _tile_sums(px[:, y0:y0 + WIN, x0:x0 + WIN], py[:, y0:y0 + WIN, x0:x0 + WIN], inside,
                              min(TILE, OH - y0), min(TILE, OW - x0), shift)
            acc[:, 0] += s
            acc[:, 1] += c
    return acc / float(OH * OW)


def _pool(v):
    """2x2 mean in fp32, odd sizes repeat the last row / column; sum order as the kernel's."""
    P, H, W = v.shape
    ya, xa = np.arange(0, H, 2), np.arange(0, W, 2)
    yb, xb = np.minimum(ya + 1, H - 1), np.minimum(xa + 1, W - 1)
    q = [v[:, yy][:, :, xx] for yy, xx in ((ya, xa), (yb, xa), (ya, xb), (yb, xb))]
    return F32(0.25) * (((q[0] + q[1]) + q[2]) + q[3])


def ms_ssim_terms(img1, img2, shift="window_mean"):
    """The (N,3,5,2) terms alone, laid out as oracle.nic_oracle.ms_ssim_terms."""
    return ms_ssim(img1, img2, shift)[1]


def ms_ssim(img1, img2, shift="window_mean"):
    """(N,H,W,3) u8 pair -> (result (N,), terms (N,3,5,2)), both fp32 as the device returns
    them: terms are (mean SSIM, mean cs) per channel and scale; the result is formed from the
    float64 means (cs of scales 0..3, SSIM of scale 4, relu'd, weighted geometric mean,
    averaged over channels)."""
    n, h, w, c = img1.shape
    x = (img1.astype(F32) * (F32(1.0) / F32(255.0))).transpose(0, 3, 1, 2).reshape(n * c, h, w)
    y = (img2.astype(F32) * (F32(1.0) / F32(255.0))).transpose(0, 3, 1, 2).reshape(n * c, h, w)
    terms = []
    for k in range(SCALES):
        if k:
            x, y = _pool(x), _pool(y)
        terms.append(_scale_terms(x, y, shift))
    t = np.stack(terms, axis=1).reshape(n, c, SCALES, 2)
    wts = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
    mcs = np.concatenate([t[:, :, :-1, 1], t[:, :, -1:, 0]], axis=-1)
    res = np.prod(np.maximum(mcs, 0) ** wts, axis=-1).mean(axis=-1)
    return res.astype(F32), t.astype(F32)
