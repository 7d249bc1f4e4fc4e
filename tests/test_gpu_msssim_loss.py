"""The MS-SSIM training loss on the GPU: nic_pool2_prep, nic_msssim_terms and their backward
kernels each against a reference at the smallest shapes that reach every path, the adjoint
identity of the pool, train_hip.ms_ssim_mean end to end, and Training(distortion="ms_ssim").

End-to-end tolerance (the yardstick of test_ssim_flat_patches_no_worse_than_fp32_reference): the
reference is the float64 restatement (tests/msssim_ref.py); on the same inputs the fp32 PyTorch
restatement (training.ms_ssim(hip=False) on the device) has an error e32 against it; the HIP
path's maximum error, for the value and for each input gradient, must be at most
2 e32 + 2^-23 max|reference|.  The per-case figures are in DESIGN section 19.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import _lib  # noqa: E402
from neural_network_image_compression_amd import train_hip  # noqa: E402
from neural_network_image_compression_amd import training as T  # noqa: E402
from tests import msssim_ref as R  # noqa: E402
from tests.test_gpu_train import TOL  # noqa: E402
from tests.test_gpu_train_domain import SSIM_GRAD_RTOL, _offset_view, _rel_err, _ssim_terms  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
C1, C2 = 0.01 ** 2, 0.03 ** 2
# 2x2, 3x3: one window, with and without the repeated row / column; 22x23, 23x22: an odd width /
# height alone, a ragged last group of four columns; 65x129: more than one block per plane row
# group; 16x24 and 17x32: widths that are multiples of 8 (the 16-byte path), even and odd height
POOL_HW = [(2, 2), (3, 3), (22, 23), (23, 22), (65, 129), (16, 24), (17, 32)]
POOL_N = [1, 3, 65]


def _report(what, *figs):
    print(f"\n[msssim-loss] {what}: " + " ".join(f"{f:.3e}" if isinstance(f, float) else str(f) for f in figs))


# ---- nic_pool2_prep ------------------------------------------------------------------------------
def _pool_f32(t):
    """The stated fp32 order on (n,h,w): 0.25 * ((a + b) + (c + d)), a, b the upper pair, the last
    row / column of an odd size repeated."""
    h, w = t.shape[1:]
    t = torch.nn.functional.pad(t[:, None], (0, w % 2, 0, h % 2), mode="replicate")[:, 0]
    return 0.25 * ((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2]))


def _ulps(a, ref):
    """max |a - ref| in units of ref's fp32 spacing."""
    a, ref = a.double().cpu(), ref.double().cpu()
    spacing = torch.ldexp(torch.ones_like(ref), torch.floor(torch.log2(ref.abs().clamp_min(1e-30))).int() - 23)
    return float(((a - ref).abs() / spacing).max())


@functools.lru_cache(maxsize=None)
def _pool_planes(n, hw):
    g = torch.Generator().manual_seed(100 * hw[0] + hw[1] + n)
    x = torch.rand((n, *hw), generator=g)
    y = (x + 0.05 * torch.randn((n, *hw), generator=g)).clamp(0, 1)
    return x, y, _pool_f32(x), _pool_f32(y)


@pytest.mark.parametrize("n", POOL_N)
@pytest.mark.parametrize("hw", POOL_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool2_prep_matches_fp32_restatement(hw, n):
    x, y, xp_ref, yp_ref = _pool_planes(n, hw)
    for view in (lambda t: t, _offset_view):  # 16-byte aligned, and one float off (scalar accesses)
        xd, yd = view(x.cuda()), view(y.cuda())
        xp, yp, p, q = train_hip.pool2_prep(xd, yd, train_hip.POOL2_PREP)
        assert tuple(xp.shape) == (n, -(-hw[0] // 2), -(-hw[1] // 2))
        assert torch.equal(xp.cpu(), xp_ref) and torch.equal(yp.cpu(), yp_ref)
        assert _ulps(p, xp_ref * yp_ref) <= 1 and _ulps(q, xp_ref * xp_ref + yp_ref * yp_ref) <= 1
        xp2, yp2 = train_hip.pool2_prep(xd, yd, train_hip.POOL2_POOL)
        assert torch.equal(xp2, xp) and torch.equal(yp2, yp)
        p0, q0 = train_hip.pool2_prep(xd, yd, train_hip.POOL2_PRODUCTS)
        assert tuple(p0.shape) == (n, *hw)
        assert _ulps(p0, x * y) <= 1 and _ulps(q0, x * x + y * y) <= 1


def test_pool2_products_mode_copies_planes_when_asked():
    x, y, _, _ = _pool_planes(3, (22, 23))
    xd, yd = x.cuda(), y.cuda()
    outs = [torch.full_like(xd, float("nan")) for _ in range(4)]
    _lib.check(_lib.lib().nic_pool2_prep(xd.data_ptr(), yd.data_ptr(), 3, 22, 23, train_hip.POOL2_PRODUCTS,
                                         *(t.data_ptr() for t in outs), torch.cuda.current_stream().cuda_stream),
               "nic_pool2_prep")
    assert torch.equal(outs[0], xd) and torch.equal(outs[1], yd)
    assert _ulps(outs[2], x * y) <= 1 and _ulps(outs[3], x * x + y * y) <= 1


# ---- nic_pool2_prep_grad ---------------------------------------------------------------------------
@pytest.mark.parametrize("hw", POOL_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool2_adjoint_identity(hw):
    # <P(u), v> = <u, P^T(v)> for the pool alone (linear); both sides summed in float64, so what is
    # left is the kernels' fp32 rounding: (h + w) 2^-23 of sum |P(u)| |v| is the derivable bound
    n = 3
    g = torch.Generator().manual_seed(hw[0] * 1000 + hw[1])
    u = torch.rand((n, *hw), generator=g).cuda()  # one sign: |P(u)| is the size of the pool's own sums
    coarse = (n, -(-hw[0] // 2), -(-hw[1] // 2))
    v, v2 = torch.randn(coarse, generator=g).cuda(), torch.randn(coarse, generator=g).cuda()
    pu, pu2 = train_hip.pool2_prep(u, u.flip(0), train_hip.POOL2_POOL)
    du, du2 = train_hip.pool2_prep_grad(v, v2, None, None, None, None, hw, train_hip.POOL2_POOL)
    for a, b, c, d in ((pu, v, u, du), (pu2, v2, u.flip(0), du2)):
        lhs, rhs = float((a.double() * b.double()).sum()), float((c.double() * d.double()).sum())
        scale = float((a.double().abs() * b.double().abs()).sum())
        _report(f"adjoint {hw}", abs(lhs - rhs) / scale, (hw[0] + hw[1]) * EPS)
        assert abs(lhs - rhs) <= (hw[0] + hw[1]) * EPS * scale


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("hw", POOL_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool2_prep_grad_matches_float64_autograd(hw, n):
    x, y, _, _ = _pool_planes(n, hw)
    g = torch.Generator().manual_seed(7 + hw[0] + n)
    coarse = (n, -(-hw[0] // 2), -(-hw[1] // 2))
    ups = [torch.randn(coarse, generator=g) for _ in range(4)]
    xr, yr = x.double().requires_grad_(), y.double().requires_grad_()
    xp, yp = R.downscale(xr[:, None])[:, 0], R.downscale(yr[:, None])[:, 0]
    outs = (xp, yp, xp * yp, xp * xp + yp * yp)
    sum((o * u.double()).sum() for o, u in zip(outs, ups)).backward()
    for view in (lambda t: t, _offset_view):
        xd, yd = view(x.cuda()).requires_grad_(), view(y.cuda()).requires_grad_()
        got = train_hip.pool2_prep_fn(xd, yd, train_hip.POOL2_PREP)
        sum((o * u.cuda()).sum() for o, u in zip(got, ups)).backward()
        ex, ey = _rel_err(xd.grad, xr.grad), _rel_err(yd.grad, yr.grad)
        # dx = f (dx' + dP y' + 2 dQ x') with f a power of two: three products and two sums of fp32
        # operands whose x', y' carry the pool's own rounding (2 eps): 8 eps of the largest gradient
        assert ex <= 8 * EPS and ey <= 8 * EPS, (hw, n, ex, ey)
    # products only (scale 0), through autograd
    xr2, yr2 = x.double().requires_grad_(), y.double().requires_grad_()
    fine = [torch.randn((n, *hw), generator=g) for _ in range(2)]
    ((xr2 * yr2 * fine[0].double()).sum() + ((xr2 * xr2 + yr2 * yr2) * fine[1].double()).sum()).backward()
    xd, yd = x.cuda().requires_grad_(), y.cuda().requires_grad_()
    p, q = train_hip.pool2_prep_fn(xd, yd, train_hip.POOL2_PRODUCTS)
    ((p * fine[0].cuda()).sum() + (q * fine[1].cuda()).sum()).backward()
    assert _rel_err(xd.grad, xr2.grad) <= 8 * EPS and _rel_err(yd.grad, yr2.grad) <= 8 * EPS


# ---- nic_msssim_terms / nic_msssim_terms_grad ---------------------------------------------------------
TERM_HW = [(1, 1), (31, 33), (32, 32), (32, 33)]  # 1, 1,023, 1,024 (= SSIM_PIX, one block), 1,056 pixels


def _terms_ref64(terms, g_ssim, g_cs):
    ts = [torch.from_numpy(t).double().requires_grad_() for t in terms]
    mx, my, sxy, sxx = ts
    num0, den0 = 2 * mx * my, mx * mx + my * my
    cs = (2 * sxy - num0 + C2) / (sxx - den0 + C2)
    lcs = (num0 + C1) / (den0 + C1) * cs
    lm, cm = lcs.mean(dim=(1, 2)), cs.mean(dim=(1, 2))
    ((lm * torch.from_numpy(g_ssim).double()).sum() + (cm * torch.from_numpy(g_cs).double()).sum()).backward()
    return lm.detach(), cm.detach(), [t.grad for t in ts]


@pytest.mark.parametrize("which", ["both", "g_ssim=0", "g_cs=0"])
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("hw", TERM_HW, ids=lambda s: f"hw{s[0] * s[1]}")
def test_msssim_terms_and_grad_match_float64(hw, n, which):
    terms, wts = _ssim_terms(n, hw)
    assert train_hip.SSIM_PIX == 1024
    g_ssim = np.zeros(n, np.float32) if which == "g_ssim=0" else wts.astype(np.float32)
    g_cs = np.zeros(n, np.float32) if which == "g_cs=0" else wts[::-1].astype(np.float32).copy()
    lm, cm, grads = _terms_ref64(terms, g_ssim, g_cs)
    gs, gc = torch.from_numpy(g_ssim).cuda(), torch.from_numpy(g_cs).cuda()
    # through autograd (the stacked, 16-byte aligned form) ...
    ts = [torch.from_numpy(t).cuda().requires_grad_() for t in terms]
    lcs, cs = train_hip.msssim_terms_mean(*ts, C1, C2)
    ((lcs * gs).sum() + (cs * gc).sum()).backward()
    runs = [(lcs, cs, [t.grad for t in ts])]
    # ... and the raw calls on planes one float off 16-byte alignment (scalar accesses)
    off = [_offset_view(torch.from_numpy(t).cuda()) for t in terms]
    runs.append((*train_hip.msssim_terms(*off, C1, C2), train_hip.msssim_terms_grad(*off, gs, gc, C1, C2)))
    for lcs, cs, got in runs:
        e_l, e_c = _rel_err(lcs, lm), _rel_err(cs, cm)
        assert e_l <= TOL and e_c <= TOL, (hw, n, e_l, e_c)
        worst = max(_rel_err(t, r) for t, r in zip(got, grads))
        _report(f"terms hw={hw[0] * hw[1]} n={n} {which}", e_l, e_c, worst)
        assert worst <= SSIM_GRAD_RTOL, (hw, n, which, worst)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # one summation order


# ---- end to end ----------------------------------------------------------------------------------------
E2E = [(3, 22, 22, 2), (3, 23, 27, 2), (2, 88, 91, 4), (6, 128, 128, 4)]


@functools.lru_cache(maxsize=None)
def _e2e_reference(n, h, w, scales):
    x, y = (t.float().double() for t in R.planes(n, h, w, seed=h * w + scales))  # fp32 values
    assert float(R.used_terms(x, y, scales).min()) > 0  # the precondition: every term positive
    wts = torch.linspace(0.5, 1.5, n, dtype=torch.float64)
    xr, yr = x.clone().requires_grad_(), y.clone().requires_grad_()
    v = R.ms_ssim(xr, yr, scales)
    (v * wts).sum().backward()
    return x, y, wts, v.detach(), xr.grad, yr.grad


def _run32(fn, x, y, wts):
    xd, yd = x.float().cuda().requires_grad_(), y.float().cuda().requires_grad_()
    v = fn(xd, yd)
    (v * wts.float().cuda()).sum().backward()
    return v.detach(), xd.grad, yd.grad


def _hold(what, hip, f32, ref):
    """The rule: max|hip - ref| <= 2 max|f32 - ref| + 2^-23 max|ref|; prints the figures first."""
    ref = ref.double().cpu()
    e_hip = float((hip.double().cpu() - ref).abs().max())
    e_32 = float((f32.double().cpu() - ref).abs().max())
    mag = float(ref.abs().max())
    _report(what, "hip", e_hip, "fp32-torch", e_32, "ratio", e_hip / max(e_32, 1e-300), "max|ref|", mag)
    assert e_hip <= 2 * e_32 + EPS * mag, (what, e_hip, e_32, mag)


@pytest.mark.parametrize("n,h,w,scales", E2E, ids=lambda v: str(v))
def test_ms_ssim_mean_value_and_gradients_hold_the_fp32_yardstick(n, h, w, scales):
    x, y, wts, v_ref, gx_ref, gy_ref = _e2e_reference(n, h, w, scales)
    hip = _run32(lambda a, b: train_hip.ms_ssim_mean(a, b, scales), x, y, wts)
    f32 = _run32(lambda a, b: T.ms_ssim(a, b, scales=scales, hip=False), x, y, wts)
    via = _run32(lambda a, b: T.ms_ssim(a, b, scales=scales, hip=True), x, y, wts)
    assert all(torch.equal(a, b) for a, b in zip(hip, via))  # training.ms_ssim(hip=True) is this path
    case = f"{n}x{h}x{w} K={scales}"
    _hold(case + " value", hip[0], f32[0], v_ref)
    _hold(case + " d/dx", hip[1], f32[1], gx_ref)
    _hold(case + " d/dy", hip[2], f32[2], gy_ref)


def test_ms_ssim_mean_negative_term_is_zero_with_finite_gradient():
    g = torch.Generator().manual_seed(7)
    x = 0.5 + 0.4 * (torch.rand((2, 1, 24, 26), generator=g, dtype=torch.float64) - 0.5)
    y = 1.0 - x
    assert float(R.used_terms(x, y, 2)[:, 0].max()) < 0
    v, gx, gy = _run32(lambda a, b: train_hip.ms_ssim_mean(a, b, 2), x, y, torch.ones(2, dtype=torch.float64))
    assert torch.equal(v, torch.zeros_like(v))
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())


def test_ms_ssim_mean_refuses_small_scales():
    x = torch.rand((1, 1, 20, 40)).cuda()
    with pytest.raises(ValueError, match="10x20"):
        train_hip.ms_ssim_mean(x, x, 2)
    with pytest.raises(ValueError, match="scales"):
        train_hip.ms_ssim_mean(x, x, 6)


def test_single_scale_ssim_is_the_shared_scale_step():
    # training.ssim(hip=True) is train_hip.ssim_scale once in POOL2_PRODUCTS mode, not a second
    # route: value and input gradients equal, bit for bit, what the raw terms calls give on the
    # four filtered planes that step produces.  (3, 1, 22, 23): the smallest planes that hold the
    # window with a block tail (12 x 13 = 156 of 1,024 pixels) and an odd width.
    x, y, _, _ = _pool_planes(3, (22, 23))
    wts = torch.tensor([1.0, -0.5, 2.0]).cuda()
    xd, yd = x.cuda()[:, None].requires_grad_(), y.cuda()[:, None].requires_grad_()
    s = T.ssim(xd, yd, hip=True)
    (s * wts).sum().backward()
    xs, ys = x.cuda().requires_grad_(), y.cuda().requires_grad_()
    g = T._gauss_window(torch, xs.device, torch.float32)
    _, _, f, lcs, _ = train_hip.ssim_scale(xs, ys, g, C1, C2, train_hip.POOL2_PRODUCTS)
    assert tuple(f.shape) == (4, 3, 12, 13)
    terms = f.detach().unbind(0)
    assert torch.equal(s.detach(), train_hip.msssim_terms(*terms, C1, C2)[0])
    assert torch.equal(s.detach(), lcs.detach())
    f.backward(torch.stack(train_hip.msssim_terms_grad(*terms, wts, torch.zeros_like(wts), C1, C2)))
    assert torch.equal(xd.grad[:, 0], xs.grad) and torch.equal(yd.grad[:, 0], ys.grad)


# ---- Training ------------------------------------------------------------------------------------------
def _imgs(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, hw, hw, 3), generator=g, dtype=torch.uint8)


def test_training_ms_ssim_hip_backend_against_torch_backend(tmp_path, monkeypatch):
    from neural_network_image_compression_amd import weights as W

    from tests.conftest import trained_weights

    # a trained codec on smooth patches: the decoded planes resemble the inputs, so the terms are
    # well inside (0, 1] and the comparison between backends is well conditioned
    w0 = trained_weights("0.01")
    rng = np.random.default_rng(11)
    a = np.cumsum(np.cumsum(rng.integers(-2, 3, (4, 32, 32, 3)), axis=1), axis=2).astype(np.float64)
    a -= a.min(axis=(1, 2, 3), keepdims=True)
    imgs = torch.from_numpy((a * 255.0 / np.maximum(a.max(axis=(1, 2, 3), keepdims=True), 1)).astype(np.uint8))
    seen = []
    real = T.ms_ssim

    def spy(x, y, scales=4, max_val=1.0, hip=False):
        seen.append((x.detach().clone(), y.detach().clone(), scales, hip))
        return real(x, y, scales, max_val, hip)

    monkeypatch.setattr(T, "ms_ssim", spy)
    out = {}
    for be in ("hip", "torch"):
        tr = T.Training(device="cuda", weights=w0, seed=0, checkpoint_dir=str(tmp_path) + "/", backend=be,
                        distortion="ms_ssim", ms_scales=2)
        out[be] = tr.losses(imgs, 0.01, flip=True)
    assert [(s[2], s[3]) for s in seen] == [(2, True), (2, True), (2, False), (2, False)]
    # the rule, on the planes the HIP backend's own codec produced
    for (x, y, _, _), key in zip(seen[:2], ("ssim0", "ssim1_each")):
        ref = R.ms_ssim(x.double().cpu(), y.double().cpu(), 2)
        assert float(R.used_terms(x.double().cpu(), y.double().cpu(), 2).min()) > 0
        f32 = real(x, y, 2, hip=False)
        hip = out["hip"][key].detach()
        if key == "ssim0":
            ref, f32 = ref.mean(), f32.mean()
        _hold(f"Training {key}", hip.reshape(-1), f32.reshape(-1), ref.reshape(-1))
    # and backend against backend, as test_hip_training_step_matches_torch_backend holds its losses
    for key in ("ssim0", "ssim1_each", "loss0", "loss1"):
        a, b = out["hip"][key].detach().double().cpu(), out["torch"][key].detach().double().cpu()
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max())), key


def test_training_default_distortion_is_unchanged(tmp_path, monkeypatch):
    from neural_network_image_compression_amd import weights as W

    seen = []
    real = T.ssim

    def spy(x, y, max_val=1.0, hip=False):
        seen.append((x.detach().clone(), y.detach().clone(), hip))
        return real(x, y, max_val, hip)

    monkeypatch.setattr(T, "ssim", spy)
    tr = T.Training(device="cuda", weights=W.seeded_weights(0, init="glorot"), seed=0,
                    checkpoint_dir=str(tmp_path) + "/")
    assert tr.distortion == "ssim"
    f = tr.losses(_imgs(2, 32, 12), 0.01, flip=True)
    assert len(seen) == 2 and seen[0][2] is True
    assert torch.equal(f["ssim0"].detach(), real(seen[0][0], seen[0][1], hip=True).mean())
    assert torch.equal(f["ssim1_each"].detach(), real(seen[1][0], seen[1][1], hip=True))


# ---- the C entry points refuse bad arguments before any launch ----------------------------------------
def test_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    E, S = _lib.NIC_EINVAL, _lib.NIC_ESHAPE
    buf = torch.full((64,), float("nan"), device="cuda")
    p = buf.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    f = ctypes.c_int64()
    assert L.nic_msssim_terms_work(3, 5000, ctypes.byref(f)) == _lib.NIC_OK and f.value == 2 * 3 * 5
    assert L.nic_msssim_terms_work(3, 0, ctypes.byref(f)) == S
    assert L.nic_msssim_terms_work(3, 10, None) == E
    assert L.nic_msssim_terms(p, p, p, p, -1, 4, C1, C2, p, p, p, 64, st) == S
    assert L.nic_msssim_terms(p, p, p, p, 1, 0, C1, C2, p, p, p, 64, st) == S
    assert L.nic_msssim_terms(p, p, p, None, 1, 4, C1, C2, p, p, p, 64, st) == E
    assert L.nic_msssim_terms(p, p, p, p, 1, 4, C1, C2, p, None, p, 64, st) == E
    assert L.nic_msssim_terms(p, p, p, p, 1, 4, C1, C2, p, p, p, 1, st) == E  # work too small
    assert "work" in _lib.last_error()
    assert L.nic_msssim_terms_grad(p, p, p, p, p, None, 1, 4, C1, C2, p, p, p, p, st) == E
    assert L.nic_msssim_terms_grad(p, p, p, p, p, p, 1, -4, C1, C2, p, p, p, p, st) == S
    assert L.nic_pool2_prep(p, p, 1, 0, 4, 0, p, p, p, p, st) == S
    assert L.nic_pool2_prep(p, p, 1 << 20, 1 << 10, 1 << 10, 0, p, p, p, p, st) == S  # n h w overflows int
    assert L.nic_pool2_prep(p, p, 1, 4, 4, 3, p, p, p, p, st) == E  # mode
    assert L.nic_pool2_prep(p, None, 1, 4, 4, 0, p, p, p, p, st) == E
    assert L.nic_pool2_prep(p, p, 1, 4, 4, 0, p, p, p, None, st) == E
    assert L.nic_pool2_prep(p, p, 1, 4, 4, 2, None, p, None, None, st) == E
    assert L.nic_pool2_prep_grad(p, p, p, p, p, p, 1, 4, -4, 0, p, p, st) == S
    assert L.nic_pool2_prep_grad(p, p, p, p, p, p, 1, 4, 4, 0, p, None, st) == E
    assert L.nic_pool2_prep_grad(p, p, p, p, None, p, 1, 4, 4, 0, p, p, st) == E  # dp without the saved x'
    assert L.nic_pool2_prep_grad(p, p, p, p, p, p, 1, 4, 4, 7, p, p, st) == E
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())  # nothing was launched: the buffer is as it was
