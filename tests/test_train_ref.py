"""The float64 references of the training side path (tests/train_ref.py), checked without a GPU.

tests/test_gpu_train_domain.py holds the HIP kernels to these references over the whole domain
of the C-ABI, so they are pinned here first: against float64 torch at the nine Keras layer
shapes of tests/test_gpu_train.py (the restatement those tests already trust), against each
other through the adjoint identity at every new case, the case tables against the dispatch
rules of csrc/nic_train.hip, and the host-only work-size entry points against the formulas."""
import ctypes

import numpy as np
import pytest

from tests import train_ref as R

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import _lib  # noqa: E402
from neural_network_image_compression_amd.train_hip import same_pad  # noqa: E402
from tests.test_gpu_train import SHAPES  # noqa: E402

RTOL = 1e-12


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def _torch_layer(kind, x, kern, bias, stride, gy):
    """Keras Conv2D / Conv2DTranspose (SAME) in float64 torch, NHWC in and out: y and the
    gradients of <y, gy> with respect to x and the kernel."""
    import torch.nn.functional as F

    xr, kr = (torch.from_numpy(t).requires_grad_() for t in (x, kern))
    br = torch.from_numpy(bias)
    xn = xr.permute(0, 3, 1, 2)
    k = kern.shape[0]
    if kind == "conv":
        (pt, pb), (pl, pr) = same_pad(x.shape[1], k, stride), same_pad(x.shape[2], k, stride)
        yr = F.conv2d(F.pad(xn, (pl, pr, pt, pb)), kr.permute(3, 2, 0, 1), br, stride=stride)
    else:
        oh, ow = x.shape[1] * stride, x.shape[2] * stride
        pt, pl = same_pad(oh, k, stride)[0], same_pad(ow, k, stride)[0]
        full = F.conv_transpose2d(xn, kr.permute(3, 2, 0, 1), stride=stride)
        full = F.pad(full, (0, max(0, pl + ow - full.shape[3]), 0, max(0, pt + oh - full.shape[2])))
        yr = full[:, :, pt:pt + oh, pl:pl + ow] + br.view(1, -1, 1, 1)
    yr = yr.permute(0, 2, 3, 1)
    yr.backward(torch.from_numpy(gy))
    return yr.detach().numpy(), xr.grad.numpy(), kr.grad.numpy()


@pytest.mark.parametrize("kind,cin,cout,k,stride,hw", SHAPES)
def test_references_equal_float64_torch_at_the_keras_shapes(kind, cin, cout, k, stride, hw):
    # pads, layouts and directions exactly as train_hip._conv_fn passes them
    rng = np.random.default_rng(k * 1000 + cin + cout)
    h, w = hw
    x = rng.standard_normal((2, h, w, cin))
    kern = rng.standard_normal((k, k, cin, cout) if kind == "conv" else (k, k, cout, cin)) / np.sqrt(k * k * cin)
    bias = 0.1 * rng.standard_normal(cout)
    if kind == "conv":
        oh, ow = -(-h // stride), -(-w // stride)
        pad = (same_pad(h, k, stride)[0], same_pad(w, k, stride)[0])
        gy = rng.standard_normal((2, oh, ow, cout))
        y = R.gather_ref(x, kern, 0, stride, pad, 0, (oh, ow), cout, bias)
        dx = R.gather_ref(gy, kern, 1, stride, pad, 1, (h, w), cin)
        dk = R.wgrad_ref(x, gy, k, k, stride, pad)
    else:
        oh, ow = h * stride, w * stride
        pad = (same_pad(oh, k, stride)[0], same_pad(ow, k, stride)[0])
        gy = rng.standard_normal((2, oh, ow, cout))
        y = R.gather_ref(x, kern, 1, stride, pad, 1, (oh, ow), cout, bias)
        dx = R.gather_ref(gy, kern, 0, stride, pad, 0, (h, w), cin)
        dk = R.wgrad_ref(gy, x, k, k, stride, pad)
    yr, dxr, dkr = _torch_layer(kind, x, kern, bias, stride, gy)
    for name, a, r in (("y", y, yr), ("dx", dx, dxr), ("dkernel", dk, dkr)):
        assert _rel(a, r) <= RTOL, (name, _rel(a, r))


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=lambda c: c.id)
def test_gather_reference_directions_are_adjoint(case):
    # <A x, g> == <x, A^T g>: A^T is the other direction with the other layout of the same
    # kernel buffer, mapping the output size back to the input size
    c = case
    rng = np.random.default_rng(sum(map(ord, c.id)))
    x = rng.standard_normal((c.n, c.h, c.w, c.cin))
    wt = rng.standard_normal((c.kh, c.kw, c.cin, c.cout) if c.layout == 0 else (c.kh, c.kw, c.cout, c.cin))
    g = rng.standard_normal((c.n,) + c.out_hw + (c.cout,))
    y = R.gather_ref(x, wt, c.layout, c.stride, c.pad, c.transposed, c.out_hw, c.cout)
    xt = R.gather_ref(g, wt, 1 - c.layout, c.stride, c.pad, 1 - c.transposed, (c.h, c.w), c.cin)
    lhs, rhs = float((y * g).sum()), float((x * xt).sum())
    assert abs(lhs) > 1.0  # (no chance cancellation behind the relative figure)
    assert abs(lhs - rhs) <= RTOL * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: c.id)
def test_wgrad_reference_is_the_kernel_gradient_of_the_gather_reference(case):
    # <gather(gat, W), dir> is linear in W: its gradient is wgrad_ref(gat, dir), so
    # <gather(gat, W), dir> == <W, wgrad_ref(gat, dir)> for any W
    c = case
    rng = np.random.default_rng(sum(map(ord, c.id)))
    gat = rng.standard_normal((c.n,) + c.gat_hw + (c.ca,))
    dirt = rng.standard_normal((c.n, c.uh, c.uw, c.cb))
    wt = rng.standard_normal((c.kh, c.kw, c.ca, c.cb))
    y = R.gather_ref(gat, wt, 0, c.stride, c.pad, 0, (c.uh, c.uw), c.cb)
    dw = R.wgrad_ref(gat, dirt, c.kh, c.kw, c.stride, c.pad)
    lhs, rhs = float((y * dirt).sum()), float((wt * dw).sum())
    assert abs(lhs) > 1.0
    assert abs(lhs - rhs) <= RTOL * abs(lhs), (lhs, rhs)


def test_case_tables_reach_every_kernel_form():
    seen = set()
    for c in R.GATHER_CASES:
        form = R.gather_form(c.cin, c.cout, c.transposed, c.stride, c.aligned)
        assert form == c.form, (c.id, form)
        assert c.cin <= 64 and c.cout <= 64 and c.kh * c.kw <= 64
        seen.add(form)
    assert seen == {(nt, vec, ph) for nt in (16, 32, 64) for vec, ph in ((False, False), (True, False), (True, True))}
    seen = set()
    for c in R.WGRAD_CASES:
        form = R.wgrad_form(c.kh, c.kw, c.ca, c.cb)
        assert form == c.form, (c.id, form)
        assert c.ca <= 64 and c.cb <= 64 and c.kh * c.kw <= 64
        seen.add(form)
    assert seen == {(na, nb) for na in (16, 32, 64) for nb in (16, 32, 64)}
    w9 = next(c for c in R.WGRAD_CASES if c.id == "w9")
    assert R.wgrad_slices(w9.n, w9.uh, w9.uw, w9.kh, w9.kw, w9.ca, w9.cb) == 8


def test_work_sizes_match_the_formulas_at_every_case():
    L = _lib.lib()
    v = ctypes.c_int64()
    for c in R.GATHER_CASES:
        assert L.nic_conv_gather_work(c.kh, c.kw, c.cin, c.cout, ctypes.byref(v)) == _lib.NIC_OK, c.id
        assert v.value == R.gather_work_bytes(c.kh, c.kw, c.cin, c.cout), c.id
    for c in R.WGRAD_CASES:
        assert L.nic_conv_wgrad_work(c.n, c.uh, c.uw, c.kh, c.kw, c.ca, c.cb, ctypes.byref(v)) == _lib.NIC_OK, c.id
        assert v.value == R.wgrad_work_floats(c.n, c.uh, c.uw, c.kh, c.kw, c.ca, c.cb), c.id
    for rows in R.ABG_ROWS:
        for cols in R.ABG_COLS:
            assert L.nic_act_bias_grad_work(rows, cols, ctypes.byref(v)) == _lib.NIC_OK
            assert v.value == R.act_bias_grad_work_floats(rows, cols), (rows, cols)
    for n in R.SSIM_N:
        for h, w in R.SSIM_HW:
            assert L.nic_msssim_terms_work(n, h * w, ctypes.byref(v)) == _lib.NIC_OK
            assert v.value == 2 * R.ssim_map_work_floats(n, h * w), (n, h * w)


def test_gauss_reference_equals_float64_torch_and_its_adjoint():
    import torch.nn.functional as F

    rng = np.random.default_rng(3)
    t = rng.standard_normal((2, 13, 17))
    for ntaps in (1, 2, 11):
        taps = rng.random(ntaps)
        tt, kt = torch.from_numpy(t)[:, None], torch.from_numpy(taps)
        for vertical in (0, 1):
            ker = kt.view(1, 1, -1, 1) if vertical else kt.view(1, 1, 1, -1)
            out = R.gauss_1d_ref(t, taps, vertical, 0)
            assert _rel(out, F.conv2d(tt, ker)[:, 0].numpy()) <= RTOL
            g = rng.standard_normal(out.shape)
            back = R.gauss_1d_ref(g, taps, vertical, 1)
            assert back.shape == t.shape
            assert abs(float((out * g).sum()) - float((t * back).sum())) <= RTOL * float(np.abs(out * g).sum())


def test_ssim_map_reference_gradient_equals_float64_autograd():
    rng = np.random.default_rng(4)
    x = rng.random((3, 9, 7))
    y = np.clip(x + 0.1 * rng.standard_normal(x.shape), 0, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    terms = [x, y, x * y, x * x + y * y]  # any positive planes serve: the map is pointwise
    g = np.array([1.0, -0.5, 2.0])
    ts = [torch.from_numpy(t).requires_grad_() for t in terms]
    mx, my, sxy, sxx = ts
    num0, den0 = mx * my * 2.0, mx * mx + my * my
    v = ((num0 + c1) / (den0 + c1)) * ((sxy * 2.0 - num0 + c2) / (sxx - den0 + c2))
    mean = v.mean(dim=(1, 2))
    assert _rel(R.ssim_map_ref(*terms, c1, c2), mean.detach().numpy()) <= RTOL
    (mean * torch.from_numpy(g)).sum().backward()
    for a, t in zip(R.ssim_map_grad_ref(*terms, g, c1, c2), ts):
        assert _rel(a, t.grad.numpy()) <= 1e-10  # the terms cancel: sxx - den0 is O(c2) here


def test_absmax_scale_reference():
    f = R.absmax_scale_ref
    assert f(np.zeros(7)) == 1.0 and f(np.zeros(0)) == 1.0
    assert f([1.0]) == 2.0 ** 13 and f([-1.5, 0.2]) == 2.0 ** 13 and f([2.0]) == 2.0 ** 12
    assert f([0.999]) == 2.0 ** 14 and f([3e-9]) == 2.0 ** (13 + 29)  # 2^-29 <= 3e-9 < 2^-28
    assert f([1.0, np.inf]) == 1.0 and f([-np.inf]) == 1.0
    # a NaN element is skipped, as fmaxf skips it: the finite maximum decides
    assert f([np.nan, 4.0, 1.0]) == 2.0 ** 11 and f([np.nan, np.nan]) == 1.0
    assert f([np.nan, np.inf]) == 1.0
    for m in (1e-30, 3.7, 65504.0, 1e30):  # max * scale in [2^13, 2^14)
        assert 2.0 ** 13 <= m * f([m]) < 2.0 ** 14
    assert f([1e-45]) == 2.0 ** 126 and f([3e38]) == 2.0 ** (13 - 127)
