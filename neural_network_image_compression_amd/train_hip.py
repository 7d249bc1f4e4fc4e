"""HIP convolutions for the training side path (tf2_0/src/training.py:74-151).

Keras ``Conv2D(padding='SAME')`` and ``Conv2DTranspose(padding='SAME')`` on NHWC fp32
tensors, forward and backward, on the split-f16x3 MFMA kernels of ``csrc/nic_train.hip``
through the C-ABI (``nic_conv_gather``, ``nic_conv_wgrad``, ``nic_absmax_scale``):

=====================  ==========================================================
Conv2D forward         gather, src = s*o + k - pad, kernel HWIO (layout 0)
Conv2D input grad      gather "transposed", src = (o + pad - k)/s, same kernel (layout 1)
Conv2D kernel grad     wgrad(gat = x, dir = dy) -> HWIO
Conv2DTranspose fwd    gather "transposed", kernel HWOI (layout 1)
Conv2DTranspose dx     gather, src = s*o + k - pad, same kernel (layout 0)
Conv2DTranspose dW     wgrad(gat = dy, dir = x) -> HWOI
=====================  ==========================================================

The SSIM loss (``ssim_mean``) and the MS-SSIM loss (``ms_ssim_mean``) share one per-scale step
(``ssim_scale``): the Gaussian's product planes, pooled between scales (``nic_pool2_prep`` and its
adjoint), the separable Gaussian over the four stacked planes (a 1-D one-channel VALID
correlation and its adjoint, ``nic_gauss_1d``) and both per-plane means of the scale in one pass
(``nic_msssim_terms`` and its backward).  The SSIM loss is that step once, on scale 0.

The table rate loss (``rate_table``, ``Training(rate="table")``) is ``nic_rate_table`` and
``nic_rate_table_grad``: per-plane code lengths under a table of -log2 p, the latent's gradient
and the table's (no atomics; each only when asked for).  The context rate loss (``rate_ctable``,
``Training(rate="context")``) is ``nic_rate_ctable`` and ``nic_rate_ctable_grad``: the same under
the one of three rows per channel that the left neighbour's code selects, what .nic version 3 prices.

Each operand gets a power-of-two scale (max |t| * scale in [2^13, 2^14)) computed on the
device once per tensor (x and the kernel in the forward, dy in the backward), so the f16 hi/lo split keeps tiny gradients exact to ~2^-22.  The layers' leaky-ReLU runs in
the gather's epilogue (``nic_conv_gather_act``), and its gradient with the bias gradient in
one deterministic pass (``nic_act_bias_grad``: dz = dy * leaky'(y), db = column sums of dz).
The clip, residual-add and noise elementwise parts and the Entropynet's two dense layers
(plain library GEMMs) stay on torch.  There is no fallback: without the built library these
raise.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Tuple

from . import _lib


def _torch():
    import torch

    return torch


def same_pad(n: int, k: int, s: int) -> Tuple[int, int]:
    out = -(-n // s)
    pad = max((out - 1) * s + k - n, 0)
    return pad // 2, pad - pad // 2


def _stream(device):
    """The current stream of the operands' device (not of the current device)."""
    return _torch().cuda.current_stream(device).cuda_stream


def _same_device(*ts):
    devs = {t.device for t in ts if t is not None}
    if len(devs) != 1:
        raise ValueError(f"operands on different devices: {sorted(map(str, devs))}")
    return devs.pop()


def scale(t):
    """Device (1,) fp32 power-of-two operand scale of t (nic_absmax_scale); computed once per
    tensor and passed to every GEMM that reads it.  Strided views are made contiguous first
    (the kernel reads t.numel() elements from t.data_ptr())."""
    torch = _torch()
    t = _check(t, "scale t")
    with torch.cuda.device(t.device):
        out = torch.empty(1, dtype=torch.float32, device=t.device)
        work = torch.empty(512, dtype=torch.float32, device=t.device)
        _lib.check(_lib.lib().nic_absmax_scale(t.data_ptr(), t.numel(), out.data_ptr(), work.data_ptr(),
                                               _stream(t.device)), "nic_absmax_scale")
    return out


def _check(t, name):
    torch = _torch()
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda":
        raise TypeError(f"{name}: expected a cuda float32 tensor")
    return t.contiguous()


def gather(x, wt, layout: int, stride: int, pad: Tuple[int, int], transposed: int, out_hw: Tuple[int, int],
           cout: int, bias=None, sx=None, sw=None, act: int = 0):
    """nic_conv_gather_act on NHWC x: returns (n, oh, ow, cout), leaky_relu(0.2)-activated
    when act.  sx / sw: operand scales (:func:`scale`), computed here when not given."""
    torch = _torch()
    import ctypes

    x = _check(x, "gather x")
    wt = _check(wt, "gather wt")
    dev = _same_device(x, wt, bias, sx, sw)
    n, h, w, cin = x.shape
    kh, kw = wt.shape[0], wt.shape[1]
    L = _lib.lib()
    need = ctypes.c_int64()
    _lib.check(L.nic_conv_gather_work(kh, kw, cin, cout, ctypes.byref(need)), "nic_conv_gather_work")
    work = torch.empty(int(need.value) // 4, dtype=torch.float32, device=x.device)
    y = torch.empty((n, out_hw[0], out_hw[1], cout), dtype=torch.float32, device=x.device)
    sx = scale(x) if sx is None else sx
    sw = scale(wt) if sw is None else sw
    bias = _check(bias, "gather bias") if bias is not None else None
    b = bias.data_ptr() if bias is not None else None
    with torch.cuda.device(dev):
        _lib.check(L.nic_conv_gather_act(x.data_ptr(), n, h, w, cin, wt.data_ptr(), kh, kw, layout, stride, pad[0],
                                         pad[1], transposed, b, sx.data_ptr(), sw.data_ptr(), y.data_ptr(), out_hw[0],
                                         out_hw[1], cout, int(act), work.data_ptr(), int(need.value), _stream(dev)),
                   "nic_conv_gather_act")
    return y


ABG_ROWS = 256  # rows per block of nic_act_bias_grad (its work: per block a row of sums and a max)


def act_bias_grad(y, dy, act: int, want_dz: bool = True, want_db: bool = True):
    """nic_act_bias_grad on NHWC tensors: (dz, db, dz_scale) with dz = dy * leaky'(y) (dy itself
    when not act), db its per-channel sums and dz_scale its operand scale (:func:`scale`), from
    one pass; dz / db are None when not wanted (dz_scale too, without dz)."""
    torch = _torch()
    dy = _check(dy, "act_bias_grad dy")
    if act:
        y = _check(y, "act_bias_grad y")
    dev = _same_device(y if act else None, dy)
    cols = dy.shape[-1]
    rows = dy.numel() // cols if cols else 0
    dz = (torch.empty_like(dy) if act else dy) if want_dz else None
    if not want_db and not want_dz:
        return None, None, None
    db = torch.empty((cols,), dtype=torch.float32, device=dy.device) if want_db else None
    sdz = torch.empty((1,), dtype=torch.float32, device=dy.device) if want_dz else None
    need = -(-rows // ABG_ROWS) * (cols + 1)  # nic_act_bias_grad_work (checked by the call)
    work = torch.empty(max(need, 1), dtype=torch.float32, device=dy.device)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nic_act_bias_grad(
            y.data_ptr() if act else None, dy.data_ptr(), rows, cols, int(act),
            dz.data_ptr() if (dz is not None and act) else None, db.data_ptr() if db is not None else None,
            sdz.data_ptr() if sdz is not None else None, work.data_ptr(), need, _stream(dev)), "nic_act_bias_grad")
    return dz, db, sdz


def wgrad(gat, dirt, kh: int, kw: int, stride: int, pad: Tuple[int, int], sg=None, sd=None):
    """nic_conv_wgrad: (kh, kw, ca, cb) = sum_u gat[s*u + k - pad][a] * dir[u][b]."""
    torch = _torch()
    import ctypes

    gat = _check(gat, "wgrad gat")
    dirt = _check(dirt, "wgrad dir")
    dev = _same_device(gat, dirt, sg, sd)
    n, gh, gw, ca = gat.shape
    _, uh, uw, cb = dirt.shape
    L = _lib.lib()
    need = ctypes.c_int64()
    _lib.check(L.nic_conv_wgrad_work(n, uh, uw, kh, kw, ca, cb, ctypes.byref(need)), "nic_conv_wgrad_work")
    work = torch.empty(max(int(need.value), 1), dtype=torch.float32, device=gat.device)
    dw = torch.empty((kh, kw, ca, cb), dtype=torch.float32, device=gat.device)
    sg = scale(gat) if sg is None else sg
    sd = scale(dirt) if sd is None else sd
    with torch.cuda.device(dev):
        _lib.check(L.nic_conv_wgrad(gat.data_ptr(), n, gh, gw, ca, dirt.data_ptr(), uh, uw, cb, kh, kw, stride,
                                    pad[0], pad[1], sg.data_ptr(), sd.data_ptr(), dw.data_ptr(), work.data_ptr(),
                                    int(need.value), _stream(dev)), "nic_conv_wgrad")
    return dw


def gauss_1d(t, taps, vertical: int, adjoint: int):
    """nic_gauss_1d on one-channel planes (n, h, w)."""
    torch = _torch()
    t = _check(t, "gauss t")
    taps = _check(taps, "gauss taps")
    dev = _same_device(t, taps)
    n, h, w = t.shape
    d = taps.numel() - 1
    sgn = 1 if adjoint else -1
    ho, wo = (h + sgn * d, w) if vertical else (h, w + sgn * d)
    out = torch.empty((n, ho, wo), dtype=torch.float32, device=t.device)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nic_gauss_1d(t.data_ptr(), n, h, w, taps.data_ptr(), taps.numel(), vertical, adjoint,
                                           out.data_ptr(), ho, wo, _stream(dev)), "nic_gauss_1d")
    return out


POOL2_PREP, POOL2_PRODUCTS, POOL2_POOL = 0, 1, 2  # nic.h NIC_POOL2_*


def pool2_prep(x, y, mode: int = POOL2_PREP):
    """nic_pool2_prep on one-channel planes (n, h, w): the MS-SSIM loss's step to the next scale.
    POOL2_PREP -> (x', y', x'y', x'x' + y'y') at (n, ceil(h/2), ceil(w/2)); POOL2_POOL -> (x', y');
    POOL2_PRODUCTS (no pooling, scale 0) -> (x y, x x + y y) at (n, h, w)."""
    torch = _torch()
    x, y = _check(x, "pool2_prep x"), _check(y, "pool2_prep y")
    dev = _same_device(x, y)
    if x.dim() != 3 or x.shape != y.shape:
        raise ValueError(f"pool2_prep: planes (n, h, w) of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    n, h, w = x.shape
    shape = (n, h, w) if mode == POOL2_PRODUCTS else (n, -(-h // 2), -(-w // 2))
    outs = [torch.empty(shape, dtype=torch.float32, device=x.device)
            for _ in range(4 if mode == POOL2_PREP else 2)]
    ptrs = [t.data_ptr() for t in outs]
    ptrs = {POOL2_PREP: ptrs, POOL2_PRODUCTS: [None, None] + ptrs, POOL2_POOL: ptrs + [None, None]}.get(mode, ptrs)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nic_pool2_prep(x.data_ptr(), y.data_ptr(), n, h, w, mode, *ptrs[:4], _stream(dev)),
                   "nic_pool2_prep")
    return tuple(outs)


def pool2_prep_grad(dxp, dyp, dp, dq, xp, yp, hw: Tuple[int, int], mode: int = POOL2_PREP):
    """nic_pool2_prep_grad: (dx, dy) at (n, h, w) = ``hw`` from the gradients of pool2_prep's
    outputs (each may be None: zero) and its saved x', y' (None without dp and dq)."""
    torch = _torch()
    ts = [None if t is None else _check(t, "pool2_prep_grad operand") for t in (dxp, dyp, dp, dq, xp, yp)]
    given = [t for t in ts if t is not None]
    if not given:
        raise ValueError("pool2_prep_grad: no operand")
    dev = _same_device(*given)
    h, w = hw
    coarse = (h, w) if mode == POOL2_PRODUCTS else (-(-h // 2), -(-w // 2))
    n = given[0].shape[0]
    for t in given:
        if tuple(t.shape) != (n, *coarse):
            raise ValueError(f"pool2_prep_grad: operand {tuple(t.shape)}, expected {(n, *coarse)}")
    dx = torch.empty((n, h, w), dtype=torch.float32, device=given[0].device)
    dy = torch.empty_like(dx)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nic_pool2_prep_grad(*(None if t is None else t.data_ptr() for t in ts), n, h, w, mode,
                                                  dx.data_ptr(), dy.data_ptr(), _stream(dev)), "nic_pool2_prep_grad")
    return dx, dy


def msssim_terms(mx, my, sxy, sxx, c1: float, c2: float):
    """nic_msssim_terms: the (n,) plane means of lum cs and of cs from one scale's filtered terms."""
    torch = _torch()
    ts = [_check(t, "msssim_terms term") for t in (mx, my, sxy, sxx)]
    dev = _same_device(*ts)
    n = ts[0].shape[0]
    hw = ts[0].numel() // max(n, 1)
    lcs = torch.empty((n,), dtype=torch.float32, device=ts[0].device)
    cs = torch.empty_like(lcs)
    need = 2 * n * (-(-hw // SSIM_PIX))  # nic_msssim_terms_work (checked by the call)
    work = torch.empty(max(need, 1), dtype=torch.float32, device=ts[0].device)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nic_msssim_terms(*(t.data_ptr() for t in ts), n, hw, c1, c2, lcs.data_ptr(),
                                               cs.data_ptr(), work.data_ptr(), need, _stream(dev)), "nic_msssim_terms")
    return lcs, cs


def msssim_terms_grad(mx, my, sxy, sxx, g_ssim, g_cs, c1: float, c2: float, out=None):
    """nic_msssim_terms_grad: the four terms' gradients of sum g_ssim mean(lum cs) + g_cs mean(cs);
    ``out``: a (4, ...) buffer to write them into (its four slices are returned)."""
    torch = _torch()
    ts = [_check(t, "msssim_terms_grad term") for t in (mx, my, sxy, sxx)]
    g_ssim, g_cs = _check(g_ssim, "msssim_terms_grad g_ssim"), _check(g_cs, "msssim_terms_grad g_cs")
    dev = _same_device(*ts, g_ssim, g_cs)
    n = ts[0].shape[0]
    hw = ts[0].numel() // max(n, 1)
    if g_ssim.numel() != n or g_cs.numel() != n:
        raise ValueError("msssim_terms_grad: one g_ssim and one g_cs per plane")
    grads = [torch.empty_like(t) for t in ts] if out is None else list(out.unbind(0))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nic_msssim_terms_grad(*(t.data_ptr() for t in ts), g_ssim.data_ptr(), g_cs.data_ptr(), n,
                                                    hw, c1, c2, *(t.data_ptr() for t in grads), _stream(dev)),
                   "nic_msssim_terms_grad")
    return tuple(grads)


RATE_PIX, RATE_SLAB = 1024, 128  # the rate forward's elements / the rate backward's pixels per block


def _rate_args(who, y, L, groups: int, anchors, seg_pixels: int, yc):
    """The checked operands of a rate call and its nic_rate_[c]table_work count.  anchors None: the
    table rate (one context per row, seg_pixels and yc unused); else the context rate (three)."""
    torch = _torch()
    y, L = _check(y, f"{who} y"), _check(L, f"{who} L")
    m, h, w, c = y.shape
    contexts = 1 if anchors is None else 3
    want = (groups * c, 256) if anchors is None else (groups * c, 3, 256)
    if tuple(L.shape) != want:
        raise ValueError(f"{who}: L must be {want} for {groups} groups of {c} channels, got {tuple(L.shape)}")
    if anchors is not None:
        if (not isinstance(anchors, torch.Tensor) or anchors.dtype != torch.uint8
                or tuple(anchors.shape) != (groups * c,) or not anchors.is_contiguous()):
            raise ValueError(f"{who}: anchors must be a contiguous ({groups * c},) torch.uint8 tensor")
        if yc is not None:
            yc = _check(yc, f"{who} yc")
            if yc.shape != y.shape:
                raise ValueError(f"{who}: yc {tuple(yc.shape)} is not y's shape {tuple(y.shape)}")
        if int(seg_pixels) < 1:
            raise ValueError(f"{who}: seg_pixels must be at least 1, not {seg_pixels}")
    dev = _same_device(y, yc, L, anchors)
    need = max(m * -(-(h * w * c) // RATE_PIX),
               contexts * groups * -(-(m // max(groups, 1) * h * w) // RATE_SLAB) * c * 256)
    return y, yc, L, dev, (m, h, w, c), need


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rate_bits(who, y, L, groups: int, anchors=None, seg_pixels: int = 1, yc=None):
    torch = _torch()
    y, yc, L, dev, (m, h, w, c), need = _rate_args(who, y, L, groups, anchors, seg_pixels, yc)
    bits = torch.empty((m,), dtype=torch.float32, device=y.device)
    work = torch.empty(max(need, 1), dtype=torch.float32, device=y.device)
    tail = (bits.data_ptr(), work.data_ptr(), need, _stream(dev))
    with torch.cuda.device(dev):
        if anchors is None:
            rc = _lib.lib().nic_rate_table(y.data_ptr(), L.data_ptr(), m, h, w, c, groups, *tail)
        else:
            rc = _lib.lib().nic_rate_ctable(y.data_ptr(), _ptr(yc), L.data_ptr(), anchors.data_ptr(), m, h, w, c, groups,
                                            int(seg_pixels), *tail)
        _lib.check(rc, f"nic_{who}")
    return bits


def _rate_grad(who, y, L, g, groups: int, want_dy: bool, want_dl: bool, anchors=None, seg_pixels: int = 1, yc=None):
    torch = _torch()
    y, yc, L, dev, (m, h, w, c), need = _rate_args(who, y, L, groups, anchors, seg_pixels, yc)
    g = _check(g, f"{who} g")
    _same_device(y, g)
    if g.numel() != m:
        raise ValueError(f"{who}: one g per plane")
    dy = torch.empty_like(y) if want_dy else None
    dl = torch.empty_like(L) if want_dl else None
    work = torch.empty(max(need, 1), dtype=torch.float32, device=y.device) if want_dl else None
    tail = (_ptr(dy), _ptr(dl), _ptr(work), need if want_dl else 0, _stream(dev))
    with torch.cuda.device(dev):
        if anchors is None:
            rc = _lib.lib().nic_rate_table_grad(y.data_ptr(), L.data_ptr(), g.data_ptr(), m, h, w, c, groups, *tail)
        else:
            rc = _lib.lib().nic_rate_ctable_grad(y.data_ptr(), _ptr(yc), L.data_ptr(), anchors.data_ptr(), g.data_ptr(),
                                                 m, h, w, c, groups, int(seg_pixels), *tail)
        _lib.check(rc, f"nic_{who}")
    return dy, dl


def rate_table_bits(y, L, groups: int):
    """nic_rate_table: the (m,) code lengths in bits of the planes of y (m, h, w, c) NHWC under the
    table L (groups * c, 256) of -log2 p."""
    return _rate_bits("rate_table", y, L, groups)


def rate_table_grad(y, L, g, groups: int, want_dy: bool = True, want_dl: bool = True):
    """nic_rate_table_grad: (dy, dL) of sum_m g[m] plane_bits[m]; one is None when not wanted (its
    pointer goes down as NULL and its kernel does not run)."""
    return _rate_grad("rate_table_grad", y, L, g, groups, want_dy, want_dl)


def rate_ctable_bits(y, L, anchors, groups: int, seg_pixels: int, yc=None):
    """nic_rate_ctable: the (m,) code lengths in bits of the planes of y (m, h, w, c) NHWC under the
    context table L (groups * c, 3, 256) of -log2 p; the row of an element is picked by its left
    neighbour's code in yc (None: y) against anchors ((groups * c,) u8), segments of seg_pixels."""
    return _rate_bits("rate_ctable", y, L, groups, _anchors(anchors), seg_pixels, yc)


def rate_ctable_grad(y, L, anchors, g, groups: int, seg_pixels: int, yc=None, want_dy: bool = True,
                     want_dl: bool = True):
    """nic_rate_ctable_grad: (dy, dL) of sum_m g[m] plane_bits[m]; one is None when not wanted (its
    pointer goes down as NULL and its kernels do not run).  yc and anchors get no gradient."""
    return _rate_grad("rate_ctable_grad", y, L, g, groups, want_dy, want_dl, _anchors(anchors), seg_pixels, yc)


def _anchors(anchors):
    """The context rate's anchors as given; a missing one as a value the operand check refuses (None
    would select the table rate)."""
    return () if anchors is None else anchors


def _conv_fn():
    torch = _torch()

    class Rate(torch.autograd.Function):
        """Per-plane code length of y (m, h, w, c) under the table L of -log2 p: anchors None, the
        table rate on L (groups * c, 256) (nic_rate_table / nic_rate_table_grad); else the context
        rate on L (groups * c, 3, 256) (nic_rate_ctable / nic_rate_ctable_grad).  A gradient nobody
        asked for is not computed, and yc and anchors never get one (the context is piecewise
        constant)."""

        @staticmethod
        def forward(ctx, y, L, groups, anchors, seg_pixels, yc):
            y, L = _check(y, "Rate y"), _check(L, "Rate L")
            yc = None if yc is None else _check(yc.detach(), "Rate yc")
            if anchors is None:
                bits = rate_table_bits(y, L, groups)
            else:
                bits = rate_ctable_bits(y, L, anchors, groups, seg_pixels, yc)
            ctx.save_for_backward(y, L, anchors, yc)
            ctx.groups, ctx.seg_pixels = groups, seg_pixels
            return bits

        @staticmethod
        def backward(ctx, g):
            y, L, anchors, yc = ctx.saved_tensors
            want_dy, want_dl = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (want_dy or want_dl):
                return None, None, None, None, None, None
            if anchors is None:
                dy, dl = rate_table_grad(y, L, g.contiguous(), ctx.groups, want_dy, want_dl)
            else:
                dy, dl = rate_ctable_grad(y, L, anchors, g.contiguous(), ctx.groups, ctx.seg_pixels, yc, want_dy, want_dl)
            return dy, dl, None, None, None, None

    class Conv2DSame(torch.autograd.Function):
        """Keras Conv2D(padding='SAME'), leaky_relu(0.2) when act, NHWC; kernel (kh, kw, Cin, Cout)."""

        @staticmethod
        def forward(ctx, x, kernel, bias, stride, act):
            x, kernel = _check(x, "Conv2DSame x"), _check(kernel, "Conv2DSame kernel")
            n, h, w, _ = x.shape
            kh, kw, _, cout = kernel.shape
            pt, pl = same_pad(h, kh, stride)[0], same_pad(w, kw, stride)[0]
            oh, ow = -(-h // stride), -(-w // stride)
            sx, sw = scale(x), scale(kernel)
            y = gather(x, kernel, 0, stride, (pt, pl), 0, (oh, ow), cout, bias, sx, sw, act=int(act))
            ctx.save_for_backward(x, kernel, sx, sw, y if act else None)
            ctx.geo = (stride, pt, pl, bool(act))
            return y

        @staticmethod
        def backward(ctx, dy):
            x, kernel, sx, sw, y = ctx.saved_tensors
            stride, pt, pl, act = ctx.geo
            dy = dy.contiguous()
            need_dz = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
            dy, db, sdy = act_bias_grad(y, dy, act, need_dz, ctx.needs_input_grad[2])
            if not need_dz:
                return None, None, db, None, None
            kh, kw, cin, _ = kernel.shape
            dx = gather(dy, kernel, 1, stride, (pt, pl), 1, (x.shape[1], x.shape[2]), cin, None, sdy, sw) \
                if ctx.needs_input_grad[0] else None
            dk = wgrad(x, dy, kh, kw, stride, (pt, pl), sx, sdy) if ctx.needs_input_grad[1] else None
            return dx, dk, db, None, None

    class Conv2DTransposeSame(torch.autograd.Function):
        """Keras Conv2DTranspose(padding='SAME'), leaky_relu(0.2) when act, NHWC; kernel (kh, kw, Cout, Cin)."""

        @staticmethod
        def forward(ctx, x, kernel, bias, stride, act):
            x, kernel = _check(x, "Conv2DTransposeSame x"), _check(kernel, "Conv2DTransposeSame kernel")
            n, h, w, _ = x.shape
            kh, kw, cout, _ = kernel.shape
            oh, ow = h * stride, w * stride
            pt, pl = same_pad(oh, kh, stride)[0], same_pad(ow, kw, stride)[0]
            sx, sw = scale(x), scale(kernel)
            y = gather(x, kernel, 1, stride, (pt, pl), 1, (oh, ow), cout, bias, sx, sw, act=int(act))
            ctx.save_for_backward(x, kernel, sx, sw, y if act else None)
            ctx.geo = (stride, pt, pl, bool(act))
            return y

        @staticmethod
        def backward(ctx, dy):
            x, kernel, sx, sw, y = ctx.saved_tensors
            stride, pt, pl, act = ctx.geo
            dy = dy.contiguous()
            need_dz = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
            dy, db, sdy = act_bias_grad(y, dy, act, need_dz, ctx.needs_input_grad[2])
            if not need_dz:
                return None, None, db, None, None
            kh, kw, _, cin = kernel.shape
            dx = gather(dy, kernel, 0, stride, (pt, pl), 0, (x.shape[1], x.shape[2]), cin, None, sdy, sw) \
                if ctx.needs_input_grad[0] else None
            dk = wgrad(dy, x, kh, kw, stride, (pt, pl), sdy, sx) if ctx.needs_input_grad[1] else None
            return dx, dk, db, None, None

    class Gauss1D(torch.autograd.Function):
        """One-channel VALID correlation along x or y with constant taps (nic_gauss_1d), the
        separable Gaussian of tf.image.ssim (the SSIM loss, training.py:119-121)."""

        @staticmethod
        def forward(ctx, t, taps, vertical):
            ctx.save_for_backward(taps)
            ctx.vertical = vertical
            return gauss_1d(t, taps, vertical, 0)

        @staticmethod
        def backward(ctx, dy):
            (taps,) = ctx.saved_tensors
            return gauss_1d(dy.contiguous(), taps, ctx.vertical, 1), None, None

    class Pool2Prep(torch.autograd.Function):
        """The MS-SSIM loss's step between scales (nic_pool2_prep / nic_pool2_prep_grad) on planes
        (n, h, w); outputs as :func:`pool2_prep` for the mode."""

        @staticmethod
        def forward(ctx, x, y, mode):
            outs = pool2_prep(x, y, mode)
            ctx.mode, ctx.hw = mode, tuple(x.shape[1:])
            ctx.set_materialize_grads(False)  # an unused output's gradient stays None: not read
            if mode == POOL2_PREP:
                ctx.save_for_backward(outs[0], outs[1])
            elif mode == POOL2_PRODUCTS:
                ctx.save_for_backward(x, y)
            return outs

        @staticmethod
        def backward(ctx, *gs):
            gs = [None if g is None else g.contiguous() for g in gs]
            if ctx.mode == POOL2_PREP:
                args = (*gs, *ctx.saved_tensors)
            elif ctx.mode == POOL2_PRODUCTS:
                args = (None, None, *gs, *ctx.saved_tensors)
            else:
                args = (*gs, None, None, None, None)
            dx, dy = pool2_prep_grad(*args, ctx.hw, ctx.mode)
            return dx, dy, None

    class MsssimTerms(torch.autograd.Function):
        """Per-plane means of lum cs and of cs from one scale's filtered terms, stacked as
        f = (mx, my, sxy, sxx): (4, N, ...) (nic_msssim_terms / nic_msssim_terms_grad); the
        gradient comes back as one such stack."""

        @staticmethod
        def forward(ctx, f, c1, c2):
            f = _check(f, "MsssimTerms terms")
            if f.shape[0] != 4:
                raise ValueError("MsssimTerms: the four terms stacked along dim 0")
            ctx.save_for_backward(f)
            ctx.consts = (c1, c2)
            ctx.set_materialize_grads(False)
            return msssim_terms(*f.unbind(0), c1, c2)

        @staticmethod
        def backward(ctx, g_ssim, g_cs):
            (f,) = ctx.saved_tensors
            n = f.shape[1]
            zero = None
            if g_ssim is None or g_cs is None:
                zero = torch.zeros((n,), dtype=torch.float32, device=f.device)
            out = torch.empty_like(f)
            msssim_terms_grad(*f.unbind(0), zero if g_ssim is None else g_ssim, zero if g_cs is None else g_cs,
                              *ctx.consts, out=out)
            return out, None, None

    return _Fns(Conv2DSame, Conv2DTransposeSame, Gauss1D, Pool2Prep, MsssimTerms, Rate)


# the autograd classes, looked up by name (callers that still index find the two convolutions first)
_Fns = namedtuple("_Fns", "Conv2DSame Conv2DTransposeSame Gauss1D Pool2Prep MsssimTerms Rate")
_FNS = None


def _fns():
    global _FNS
    if _FNS is None:
        _FNS = _conv_fn()
    return _FNS


def conv_same(x, kernel_hwio, bias, stride: int, act: bool = True):
    """Keras Conv2D(padding='SAME') + leaky_relu(0.2) on NHWC (HIP, activation in the epilogue)."""
    return _fns().Conv2DSame.apply(x, kernel_hwio, bias, stride, bool(act))


def tconv_same(x, kernel_hwoi, bias, stride: int):
    """Keras Conv2DTranspose(padding='SAME') + leaky_relu(0.2) on NHWC (HIP, activation in the epilogue)."""
    return _fns().Conv2DTransposeSame.apply(x, kernel_hwoi, bias, stride, True)


def rate_table(y, L, groups: int):
    """The (m,) code lengths in bits of the planes of y (m, h, w, c) NHWC under the table L
    (groups * c, 256) of -log2 p, plane i reading the rows of group i // (m / groups) (HIP,
    differentiable in y and in L; training.table_rate states the formula)."""
    return _fns().Rate.apply(y, L, int(groups), None, 1, None)


def rate_ctable(y, L, anchors, groups: int, seg_pixels: int, yc=None):
    """The (m,) code lengths in bits of the planes of y (m, h, w, c) NHWC under the context table L
    (groups * c, 3, 256) of -log2 p: an element reads the row its left neighbour's code in yc (None:
    y) selects against anchors ((groups * c,) u8), a segment's first pixel row 0 (HIP,
    differentiable in y and in L, never in yc or anchors; training.context_rate states the formula)."""
    return _fns().Rate.apply(y, L, int(groups), _anchors(anchors), int(seg_pixels), yc)


SSIM_PIX = 1024  # map pixels per block of nic_msssim_terms (its work: two partial sums per block)


def gauss_valid(t, g1d):
    """Separable VALID Gaussian of NCHW one-channel planes (N,1,H,W) on the HIP 1-D kernel
    (horizontal then vertical, as training.ssim's filt): returns (N,1,H-10,W-10)."""
    n, c, h, w = t.shape
    if c != 1:
        raise ValueError("gauss_valid: one-channel planes")
    g1d = g1d.contiguous()
    x = _fns().Gauss1D.apply(t.reshape(n, h, w), g1d, 0)
    x = _fns().Gauss1D.apply(x, g1d, 1)
    return x.reshape(n, 1, x.shape[1], x.shape[2])


def pool2_prep_fn(x, y, mode: int = POOL2_PREP):
    """:func:`pool2_prep`, differentiable."""
    return _fns().Pool2Prep.apply(x, y, mode)


def msssim_terms_mean(mx, my, sxy, sxx, c1: float, c2: float):
    """(N,) plane means of lum cs and of cs from one scale's filtered terms (HIP, differentiable)."""
    return _fns().MsssimTerms.apply(_torch().stack([mx, my, sxy, sxx]), float(c1), float(c2))


def ssim_map_mean(mx, my, sxy, sxx, c1: float, c2: float):
    """(N,) per-plane mean of tf.image.ssim's map from its filtered terms (HIP, differentiable)."""
    return msssim_terms_mean(mx, my, sxy, sxx, c1, c2)[0]


def ssim_scale(xs, ys, g, c1: float, c2: float, mode: int):
    """One scale of the SSIM / MS-SSIM loss on planes (n, h, w), differentiable: one nic_pool2_prep
    (POOL2_PRODUCTS: the product planes of xs, ys themselves, scale 0; POOL2_PREP: pooled first),
    one Gaussian over the four stacked planes (nic_gauss_1d, twice) and nic_msssim_terms.  Returns
    (xs', ys', f, lcs, cs): this scale's planes, their filtered terms (mx, my, sxy, sxx) stacked
    (4, n, h' - 10, w' - 10), and the (n,) plane means of lum cs and of cs."""
    if mode == POOL2_PRODUCTS:
        p, q = pool2_prep_fn(xs, ys, mode)
    else:
        xs, ys, p, q = pool2_prep_fn(xs, ys, mode)
    f = _torch().cat([xs, ys, p, q], dim=0)  # one Gaussian over the four planes
    f = _fns().Gauss1D.apply(_fns().Gauss1D.apply(f, g, 0), g, 1)
    f = f.view(4, xs.shape[0], f.shape[1], f.shape[2])
    lcs, cs = _fns().MsssimTerms.apply(f, c1, c2)
    return xs, ys, f, lcs, cs


def _ssim_planes(who, x, y, max_val):
    torch = _torch()
    from .training import _gauss_window

    n, c, h, w = x.shape
    if c != 1 or y.shape != x.shape:
        raise ValueError(f"{who}: two one-channel planes (N,1,H,W) of one shape")
    g = _gauss_window(torch, x.device, torch.float32)
    return x.reshape(n, h, w), y.reshape(n, h, w), g, (0.01 * max_val) ** 2, (0.03 * max_val) ** 2


def ssim_mean(x, y, max_val: float = 1.0):
    """tf.image.ssim(x, y, max_val) of one-channel NCHW planes (N,1,H,W) -> (N,), differentiable, on
    HIP: :func:`ssim_scale` once, on the planes themselves; the plane mean of lum cs."""
    xs, ys, g, c1, c2 = _ssim_planes("ssim_mean", x, y, max_val)
    return ssim_scale(xs, ys, g, c1, c2, POOL2_PRODUCTS)[3]


def ms_ssim_mean(x, y, scales: int, max_val: float = 1.0):
    """tf.image.ssim_multiscale(x, y, max_val, power_factors=MSSSIM_WEIGHTS[:scales]) of one-channel
    NCHW planes (N,1,H,W) -> (N,), differentiable, on HIP: :func:`ssim_scale` per scale; the
    N x scales combination stays on torch."""
    from .training import ms_ssim_combine, ms_ssim_sizes

    xs, ys, g, c1, c2 = _ssim_planes("ms_ssim_mean", x, y, max_val)
    ms_ssim_sizes(xs.shape[1], xs.shape[2], scales)
    terms = []
    for k in range(scales):
        xs, ys, _, lcs, cs = ssim_scale(xs, ys, g, c1, c2, POOL2_PREP if k else POOL2_PRODUCTS)
        terms.append(lcs if k == scales - 1 else cs)
    return ms_ssim_combine(_torch().stack(terms, dim=1), scales)


def keras_adam_alpha(step: int, lr: float = 1e-4, beta1: float = 0.9, beta2: float = 0.999) -> float:
    """alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t) in fp32, with Keras' fp32 iteration powers
    (``local_step = iterations + 1``; ``pow(beta, local_step)``) -- the scalar of TF's ApplyAdam."""
    import numpy as np

    f = np.float32
    b1p, b2p = np.power(f(beta1), f(step)), np.power(f(beta2), f(step))
    return float(f(f(lr) * np.sqrt(f(1) - b2p)) / (f(1) - b1p))


class KerasAdam:
    """tf.keras.optimizers.Adam(lr) (training.py:149) on HIP: one ``nic_adam_keras`` launch per
    step over every parameter of the model (m and v kept per parameter, zero-initialised like
    Keras' slots), the update in TF's ApplyAdam order in fp32.  ``step(grads)`` takes the
    gradients in the order of ``params``."""

    def __init__(self, params, lr: float = 1e-4, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-7):
        torch = _torch()
        self.params = list(params)
        dev = _same_device(*self.params)
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("KerasAdam: parameters must be contiguous float32 tensors")
        self.lr, self.beta1, self.beta2, self.epsilon = lr, beta1, beta2, epsilon
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.iterations = 0
        self.device = dev
        self.max_n = max((p.numel() for p in self.params), default=0)
        # the {var, m, v, grad, n} table: a pinned host copy (only the gradient pointers change
        # between steps) and its device twin, reused every step
        import numpy as np

        n = len(self.params)
        self._host = torch.empty((n, 5), dtype=torch.int64, pin_memory=True)
        self._hnp = self._host.numpy()
        self._fill_table()
        self._dev = torch.empty((n, 5), dtype=torch.int64, device=dev)
        self._copied = None  # event: the last table upload has read the pinned buffer

    def _fill_table(self) -> None:
        for i, (p, m, v) in enumerate(zip(self.params, self.m, self.v)):
            self._hnp[i] = (p.data_ptr(), m.data_ptr(), v.data_ptr(), 0, p.numel())
        self._ptrs = [p.data_ptr() for p in self.params]

    def _check_table(self) -> None:
        """A parameter rebound since the table was built (p.data = ..., a reload into new
        tensors) would leave the kernel writing through a stale pointer: re-point the table
        at the current storage (same shapes: the m / v slots still fit)."""
        torch = _torch()
        if all(p.data_ptr() == q for p, q in zip(self.params, self._ptrs)):
            return
        for p, m in zip(self.params, self.m):
            if p.shape != m.shape or p.dtype != torch.float32 or not p.is_contiguous() or p.device != m.device:
                raise TypeError("KerasAdam: a parameter was rebound to a tensor of another shape / dtype / "
                                "layout / device")
        self._fill_table()

    def step(self, grads) -> None:
        torch = _torch()
        grads = [g.detach().contiguous() for g in grads]
        if len(grads) != len(self.params):
            raise ValueError("KerasAdam.step: one gradient per parameter")
        for p, g in zip(self.params, grads):
            if g.shape != p.shape or g.dtype != torch.float32 or g.device != p.device:
                raise ValueError("KerasAdam.step: gradient shape / dtype / device differs from its parameter")
        self.iterations += 1
        alpha = keras_adam_alpha(self.iterations, self.lr, self.beta1, self.beta2)
        with torch.cuda.device(self.device):
            if self._copied is not None:
                self._copied.synchronize()  # the previous upload has read the pinned table
            self._check_table()
            for i, g in enumerate(grads):
                self._hnp[i, 3] = g.data_ptr()
            self._dev.copy_(self._host, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
            _lib.check(_lib.lib().nic_adam_keras(self._dev.data_ptr(), len(grads), self.max_n, alpha, self.beta1,
                                                 self.beta2, self.epsilon, _stream(self.device)), "nic_adam_keras")
        self._keep = grads  # alive until the stream has run the launch
