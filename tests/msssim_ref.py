"""Float64 reference of the MS-SSIM training loss, written from its definition
(tf.image.ssim_multiscale on one-channel planes), independent of training.ms_ssim:

* per scale the 11x11 Gaussian (sigma 1.5) as one 2-D VALID correlation, k1 0.01, k2 0.03;
* between scales an odd height / width SYMMETRIC-padded by one on the far side (its last
  row / column repeated), then a 2x2 average pool, stride 2: each scale is ceil(previous / 2);
* scales 0 .. K-2 give the plane mean of cs, scale K-1 that of lum cs; each is clamped at 0,
  raised to MSSSIM_WEIGHTS[k] (not renormalised), and the K are multiplied;
* a term <= 0 contributes 0 and passes no gradient (not the inf / nan of pow at 0).

Gradients come from autograd on these float64 tensors.
"""
import numpy as np
import torch
import torch.nn.functional as F

MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WINDOW = 11


def window2d():
    c = np.arange(WINDOW, dtype=np.float64) - (WINDOW - 1) / 2.0
    g = np.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2 * 1.5 ** 2))
    return torch.from_numpy(g / g.sum()).view(1, 1, WINDOW, WINDOW)


def scale_terms(x, y, max_val=1.0):
    """(N,) plane means of lum cs and of cs at one scale; x, y (N,1,H,W) float64."""
    win = window2d()
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mx, my = F.conv2d(x, win), F.conv2d(y, win)
    sxy, sxx = F.conv2d(x * y, win), F.conv2d(x * x + y * y, win)
    lum = (2 * mx * my + c1) / (mx * mx + my * my + c1)
    cs = (2 * sxy - 2 * mx * my + c2) / (sxx - (mx * mx + my * my) + c2)
    return (lum * cs).mean(dim=(1, 2, 3)), cs.mean(dim=(1, 2, 3))


def downscale(t):
    """SYMMETRIC pad of odd sizes by one on the far side, then the 2x2 mean, stride 2."""
    t = F.pad(t, (0, t.shape[3] % 2, 0, t.shape[2] % 2), mode="replicate")
    return F.avg_pool2d(t, 2)


def terms(x, y, scales, max_val=1.0):
    """(N, scales, 2): per scale the plane means (lum cs, cs), before the clamp and the powers."""
    assert x.dtype == torch.float64 and y.dtype == torch.float64 and x.shape[1] == 1
    out = []
    for k in range(scales):
        if k:
            x, y = downscale(x), downscale(y)
        assert min(x.shape[2:]) >= WINDOW, (k, tuple(x.shape))
        out.append(torch.stack(scale_terms(x, y, max_val), dim=1))
    return torch.stack(out, dim=1)


def used_terms(x, y, scales, max_val=1.0):
    """(N, scales): cs of scales 0 .. K-2 and lum cs of scale K-1."""
    t = terms(x, y, scales, max_val)
    return torch.cat([t[:, :-1, 1], t[:, -1:, 0]], dim=1)


def combine(t):
    """prod_k max(t_k, 0) ** w_k with no gradient through a term <= 0."""
    w = torch.tensor(MSSSIM_WEIGHTS[:t.shape[1]], dtype=t.dtype)
    out = torch.ones(t.shape[0], dtype=t.dtype)
    for k in range(t.shape[1]):
        pos = t[:, k] > 0
        safe = torch.where(pos, t[:, k], torch.ones_like(t[:, k]))
        out = out * torch.where(pos, torch.pow(safe, w[k]), torch.zeros_like(safe))
    return out


def ms_ssim(x, y, scales, max_val=1.0):
    """(N,) = tf.image.ssim_multiscale(x, y, max_val, power_factors=MSSSIM_WEIGHTS[:scales])."""
    return combine(used_terms(x, y, scales, max_val))


def planes(n, h, w, seed, noise=0.05):
    """Seeded test planes (N,1,H,W) float64 in [0,1]: x smooth plus texture, y = clip(x + noise
    * normal), so every scale's term is positive."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, h, dtype=torch.float64).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w, dtype=torch.float64).view(1, 1, 1, w)
    ph = torch.rand((n, 1, 1, 1), generator=g, dtype=torch.float64)
    smooth = 0.5 + 0.3 * torch.sin(2 * np.pi * (yy + ph)) * torch.cos(2 * np.pi * (xx * 1.5 + ph))
    x = (smooth + 0.15 * (torch.rand((n, 1, h, w), generator=g, dtype=torch.float64) - 0.5)).clamp(0, 1)
    y = (x + noise * torch.randn((n, 1, h, w), generator=g, dtype=torch.float64)).clamp(0, 1)
    return x, y
