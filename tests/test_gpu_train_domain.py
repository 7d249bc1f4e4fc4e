"""The training GEMMs and their side kernels over every tile form and the C-ABI's full domain.

tests/test_gpu_train.py holds csrc/nic_train.hip to float64 at the nine Keras layer shapes of
the training step.  include/nic.h allows much more -- cin, cout <= 64, kh * kw <= 64, any
stride and pads, any output size, either weight layout and direction, cols <= 64 -- and the
launchers dispatch on all of it.  The tables of tests/train_ref.py hold the smallest shapes that
reach each kernel form and each branch inside it (column "reaches"; the forms are checked
against the dispatch rules in tests/test_train_ref.py); here they run against the float64
references written from the header.

The bound is the project's own, TOL = 2e-5 of tests/test_gpu_train.py: max |error| <=
TOL x max |reference| per tensor.

Measured on the MI355X, max |error| / max |reference| (deterministic; pytest -s prints them).
No case exposed a defect in a kernel or launcher.
  gather, plain / with bias and leaky-ReLU, form <NT,VEC,PH>:
     g1 <16,F,F> 1.3e-7 / 1.5e-7    g2 <16,F,F> 1.7e-7 / 1.7e-7    g3 <16,T,F> 2.2e-7 / 2.1e-7
     g4 <32,F,F> 1.3e-7 / 1.3e-7    g5 <64,F,F> 2.3e-7 / 2.1e-7    g6 <64,T,F> 1.5e-7 / 2.1e-7
     g7 <64,T,T> 2.9e-7 / 2.9e-7    g8 <64,T,T> 2.1e-7 / 1.6e-7   g9a <64,F,F> 2.9e-7 / 2.6e-7
    g9b <64,F,F> 4.9e-7 / 4.7e-7   g10 <16,F,F> 8.3e-8 / 8.4e-8   g11 <32,T,T> 2.7e-7 / 2.8e-7
    g12 <16,T,T> 1.1e-7 / 1.5e-7   g13 <32,T,F> 1.8e-7 / 1.8e-7
  wgrad, form <NA,NB> (each bit-identical on a second call):
     w1 <16,16> 9.6e-8    w2 <16,32> 1.5e-7    w3 <16,64> 1.6e-7    w4 <32,16> 1.2e-7
     w5 <64,16> 1.9e-7    w6 <64,64> 1.5e-7    w7 <64,32> 9.6e-8    w8 <64,64> 1.7e-7
     w9 <64,32> 1.4e-7   w10 <32,32> 1.2e-7   w11 <32,64> 1.6e-7
  act_bias_grad db, worst over the four row counts and both alignments, by cols (dz and dz_scale exact):
      3: 1.4e-7    5: 2.6e-7   20: 2.1e-7   50: 1.9e-7   63: 1.8e-7    4: 5.5e-7   12: 3.1e-7   60: 2.2e-7
  gauss_1d, worst over both axes and both directions, by ntaps:
      1: 0    2: 3.0e-8    11: 1.6e-7    64: 3.6e-7    11 on (2, 11, 11) planes: 1.2e-7
  ssim_map mean / worst of its four gradients (bound 1e-4), n = 1 | n = 65 (train_hip.ssim_map_mean:
  the lum cs mean of nic_msssim_terms and nic_msssim_terms_grad with g_cs = 0):
      hw 1:    3.2e-8 / 1.4e-7 | 3.3e-7 / 3.0e-6      hw 1023: 4.3e-8 / 5.2e-6 | 8.5e-8 / 4.9e-6
      hw 1024: 4.5e-8 / 5.0e-6 | 5.6e-8 / 4.2e-6      hw 1025: 3.8e-9 / 4.5e-6 | 8.7e-8 / 4.1e-6
  absmax_scale: exact in every case.  Guard bands (g5, g7, w6 and w6's partials): untouched, every
  output element written.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import train_ref as R

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import _lib  # noqa: E402
from neural_network_image_compression_amd import train_hip  # noqa: E402
from tests.test_gpu_train import TOL  # noqa: E402

pytestmark = pytest.mark.gpu

SSIM_GRAD_RTOL = 1e-4  # the figure of test_ssim_map_fused_matches_float64_both_inputs
SENTINEL = 0x7FC5A5A5  # a quiet NaN with a payload no kernel produces


def _rel_err(a, ref):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def _report(what, err):
    print(f"\n[train-domain] {what}: max|error|/max|reference| {err:.2e}")


def _offset_view(t):
    """A contiguous copy of t one float into a larger device buffer: 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ---- gather ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gather_operands(cid):
    """Seeded operands of a gather case (host fp32) and its float64 references without and with
    bias + activation; computed once, never modified."""
    c = next(k for k in R.GATHER_CASES if k.id == cid)
    g = torch.Generator().manual_seed(1000 + sum(map(ord, cid)))
    x = torch.randn((c.n, c.h, c.w, c.cin), generator=g)
    wshape = (c.kh, c.kw, c.cin, c.cout) if c.layout == 0 else (c.kh, c.kw, c.cout, c.cin)
    wt = torch.randn(wshape, generator=g) * (1.0 / np.sqrt(c.kh * c.kw * c.cin))
    bias = torch.randn((c.cout,), generator=g) * 0.1
    refs = tuple(R.gather_ref(x.numpy(), wt.numpy(), c.layout, c.stride, c.pad, c.transposed, c.out_hw, c.cout,
                              bias.numpy() if act else None, act) for act in (0, 1))
    return c, x, wt, bias, refs


@pytest.mark.parametrize("act", [0, 1], ids=["plain", "bias_act"])
@pytest.mark.parametrize("cid", [c.id for c in R.GATHER_CASES])
def test_gather_matches_float64(cid, act):
    c, x, wt, bias, refs = _gather_operands(cid)
    xd = x.cuda() if c.aligned else _offset_view(x.cuda())
    assert (xd.data_ptr() % 16 == 0) == c.aligned
    y = train_hip.gather(xd, wt.cuda(), c.layout, c.stride, c.pad, c.transposed, c.out_hw, c.cout,
                         bias.cuda() if act else None, act=act)
    torch.cuda.synchronize()
    err = _rel_err(y, refs[act])
    _report(f"gather {cid} <{c.form[0]},{'T' if c.form[1] else 'F'},{'T' if c.form[2] else 'F'}> act={act}", err)
    assert err <= TOL, (cid, act, err)


# ---- weight gradient ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wgrad_operands(cid):
    c = next(k for k in R.WGRAD_CASES if k.id == cid)
    g = torch.Generator().manual_seed(2000 + sum(map(ord, cid)))
    gat = torch.randn((c.n,) + c.gat_hw + (c.ca,), generator=g)
    dirt = torch.randn((c.n, c.uh, c.uw, c.cb), generator=g)
    return c, gat, dirt, R.wgrad_ref(gat.numpy(), dirt.numpy(), c.kh, c.kw, c.stride, c.pad)


@pytest.mark.parametrize("cid", [c.id for c in R.WGRAD_CASES])
def test_wgrad_matches_float64_and_is_deterministic(cid):
    c, gat, dirt, ref = _wgrad_operands(cid)
    gd, dd = gat.cuda(), dirt.cuda()
    dw = train_hip.wgrad(gd, dd, c.kh, c.kw, c.stride, c.pad)
    again = train_hip.wgrad(gd, dd, c.kh, c.kw, c.stride, c.pad)
    torch.cuda.synchronize()
    err = _rel_err(dw, ref)
    _report(f"wgrad {cid} <{c.form[0]},{c.form[1]}>", err)
    assert err <= TOL, (cid, err)
    assert torch.equal(dw, again), cid


# ---- activation + bias gradient ----------------------------------------------------------------
@pytest.mark.parametrize("rows", R.ABG_ROWS)
@pytest.mark.parametrize("cols", R.ABG_COLS)
def test_act_bias_grad_columns_and_row_tails(cols, rows):
    # cols / V column groups per row lane with 256 % (cols / V) != 0 (idle threads), row counts
    # either side of the 256-row block; the aligned call (V = 4 when cols % 4 == 0) and the
    # one-float-offset view (V = 1)
    g = torch.Generator().manual_seed(3000 + 100 * cols + rows)
    y = torch.randn((rows, cols), generator=g)
    y[torch.rand((rows, cols), generator=g) < 0.05] = 0.0  # y = 0 takes the 0.2 side: !(y > 0)
    dy = torch.randn((rows, cols), generator=g)
    dz_ref, db_ref = R.act_bias_grad_ref(y.numpy(), dy.numpy(), 1, np.float32)
    worst = 0.0
    for view in (lambda t: t, _offset_view):
        dz, db, sdz = train_hip.act_bias_grad(view(y.cuda()), view(dy.cuda()), 1)
        torch.cuda.synchronize()
        assert np.array_equal(dz.cpu().numpy(), dz_ref), (cols, rows)
        err = _rel_err(db, db_ref)
        worst = max(worst, err)
        assert err <= TOL, (cols, rows, err)
        assert torch.equal(sdz, train_hip.scale(dz))
        assert float(sdz) == R.absmax_scale_ref(dz_ref)
    _report(f"act_bias_grad db cols={cols} rows={rows}", worst)


# ---- separable Gaussian --------------------------------------------------------------------------
def _taps(ntaps):
    if ntaps == 64:  # random positive taps summing to 1
        t = np.random.default_rng(64).random(64) + 0.05
        return t / t.sum()
    return R.gauss_window(ntaps)


@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("vertical", [0, 1])
@pytest.mark.parametrize("ntaps,shape", [(1, (3, 70, 67)), (2, (3, 70, 67)), (11, (3, 70, 67)), (64, (3, 70, 67)),
                                         (11, (2, 11, 11))])
def test_gauss_1d_matches_float64(ntaps, shape, vertical, adjoint):
    g = torch.Generator().manual_seed(4000 + ntaps)
    t = torch.rand(shape, generator=g)
    taps = torch.from_numpy(_taps(ntaps).astype(np.float32))
    # the 11 x 11 planes: the other axis next, down to a 1 x 1 output (and, adjoint, up from one)
    if shape == (2, 11, 11):
        axes = (vertical, 1 - vertical)
        if adjoint:
            t = t[:, :1, :1].contiguous()
    else:
        axes = (vertical,)
    worst = 0.0
    for vert in axes:
        out = train_hip.gauss_1d(t.cuda(), taps.cuda(), vert, adjoint)
        torch.cuda.synchronize()
        err = _rel_err(out, R.gauss_1d_ref(t.numpy(), taps.numpy(), vert, adjoint))
        worst = max(worst, err)
        assert err <= TOL, (ntaps, shape, vert, adjoint, err)
        t = out.cpu()
    if shape == (2, 11, 11):
        assert tuple(t.shape) == ((2, 11, 11) if adjoint else (2, 1, 1))
    _report(f"gauss_1d ntaps={ntaps} planes={shape} vertical={vertical} adjoint={adjoint}", worst)


# ---- SSIM map --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ssim_terms(n, hw):
    """The four filtered terms as training.ssim builds them (two images in [0, 1], 11-tap
    Gaussian, VALID), filtered in float64 and rounded to fp32: (n, h, w) each."""
    h, w = hw
    g = torch.Generator().manual_seed(5000 + 7 * n + h * w)
    x = torch.rand((n, h + 10, w + 10), generator=g).double().numpy()
    y = np.clip(x + 0.1 * torch.randn((n, h + 10, w + 10), generator=g).double().numpy(), 0.0, 1.0)
    win = R.gauss_window()

    def filt(t):
        return R.gauss_1d_ref(R.gauss_1d_ref(t, win, 0, 0), win, 1, 0).astype(np.float32)

    terms = (filt(x), filt(y), filt(x * y), filt(x * x + y * y))
    wts = torch.randn((n,), generator=g).double().numpy()
    return terms, wts


@pytest.mark.parametrize("n", R.SSIM_N)
@pytest.mark.parametrize("hw", R.SSIM_HW, ids=lambda s: f"hw{s[0] * s[1]}")
def test_ssim_map_block_edges_and_many_planes(hw, n):
    terms, wts = _ssim_terms(n, hw)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    den0 = terms[0].astype(np.float64) ** 2 + terms[1].astype(np.float64) ** 2
    assert float((terms[3] - den0).min()) > -c2 / 2  # the inputs are a real SSIM's: the cs denominator is positive
    ts = [torch.from_numpy(t).cuda().requires_grad_() for t in terms]
    mean = train_hip.ssim_map_mean(*ts, c1, c2)
    (mean * torch.from_numpy(wts).float().cuda()).sum().backward()
    torch.cuda.synchronize()
    w32 = wts.astype(np.float32)
    err = _rel_err(mean, R.ssim_map_ref(*terms, c1, c2))
    _report(f"ssim_map mean n={n} hw={hw[0] * hw[1]}", err)
    assert err <= TOL, (n, hw, err)
    worst = 0.0
    for name, t, ref in zip(("mx", "my", "sxy", "sxx"), ts, R.ssim_map_grad_ref(*terms, w32, c1, c2)):
        e = _rel_err(t.grad, ref)
        worst = max(worst, e)
        assert e <= SSIM_GRAD_RTOL, (n, hw, name, e)
    _report(f"ssim_map_grad n={n} hw={hw[0] * hw[1]}", worst)


# ---- operand scale -----------------------------------------------------------------------------
def _scale_cases():
    g = torch.Generator().manual_seed(6000)
    base = torch.randn(1001, generator=g)
    inf, nan, ninf = base.clone(), base.clone(), base.clone()
    inf[517], nan[517], ninf[1000] = float("inf"), float("nan"), float("-inf")
    last = torch.full((1027,), 0.25)
    last[-1] = -300.0  # the maximum is the last element of an odd count: the scalar tail
    cases = {"zeros": torch.zeros(1000), "inf": inf, "neg_inf_last": ninf, "nan_among_finite": nan,
             "all_nan": torch.full((9,), float("nan")), "max_last_of_odd_count": last}
    for count in (0, 1, 3, 5):
        cases[f"count{count}"] = base[:count] * 3.0
    return cases


@pytest.mark.parametrize("name,aligned", [(k, a) for k in _scale_cases() for a in (True, False)
                                          if a or k != "count0"])  # (nothing to misalign in an empty tensor)
def test_absmax_scale_rule(name, aligned):
    # the rule of include/nic.h: 2^(13 - floor(log2 max|x|)), 1 for a zero or infinite maximum; a
    # NaN element is skipped by the maximum (fmaxf), so the finite elements beside it keep their
    # scale and a tensor of NaNs alone gets 1
    t = _scale_cases()[name]
    if name.startswith("max_last"):
        assert t.numel() == 1027 and float(t.abs().max()) == 300.0
    want = R.absmax_scale_ref(t.numpy())
    td = t.cuda() if aligned else _offset_view(t.cuda())
    got = float(train_hip.scale(td))
    assert got == want, (name, got, want)


# ---- guard bands: raw C-ABI calls writing inside a larger allocation -----------------------------
BAND = 64


def _banded(numel):
    """An int32 device buffer of sentinels and the fp32 view of its middle `numel` elements."""
    buf = torch.full((numel + 2 * BAND,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[BAND:BAND + numel].view(torch.float32)


def _check_bands(buf, numel, what):
    host = buf.cpu().numpy().view(np.uint32)
    assert np.all(host[:BAND] == SENTINEL), f"{what}: wrote below the output"
    assert np.all(host[BAND + numel:] == SENTINEL), f"{what}: wrote past the output"
    assert not np.any(host[BAND:BAND + numel] == SENTINEL), f"{what}: an output element was not written"


@pytest.mark.parametrize("cid", ["g5", "g7"])
def test_gather_writes_all_of_its_output_and_nothing_else(cid):
    c, x, wt, bias, refs = _gather_operands(cid)
    L = _lib.lib()
    xd, wd, bd = x.cuda(), wt.cuda(), bias.cuda()
    sx, sw = train_hip.scale(xd), train_hip.scale(wd)
    need = ctypes.c_int64()
    _lib.check(L.nic_conv_gather_work(c.kh, c.kw, c.cin, c.cout, ctypes.byref(need)), "nic_conv_gather_work")
    work = torch.empty(need.value // 4, dtype=torch.float32, device="cuda")
    numel = c.n * c.out_hw[0] * c.out_hw[1] * c.cout
    buf, y = _banded(numel)
    _lib.check(L.nic_conv_gather_act(xd.data_ptr(), c.n, c.h, c.w, c.cin, wd.data_ptr(), c.kh, c.kw, c.layout, c.stride,
                                     c.pad[0], c.pad[1], c.transposed, bd.data_ptr(), sx.data_ptr(), sw.data_ptr(),
                                     y.data_ptr(), c.out_hw[0], c.out_hw[1], c.cout, 1, work.data_ptr(), need.value,
                                     torch.cuda.current_stream().cuda_stream), "nic_conv_gather_act")
    torch.cuda.synchronize()
    _check_bands(buf, numel, cid)
    assert _rel_err(y.view(c.n, *c.out_hw, c.cout), refs[1]) <= TOL


def test_wgrad_writes_all_of_its_output_and_nothing_else():
    c, gat, dirt, ref = _wgrad_operands("w6")
    L = _lib.lib()
    gd, dd = gat.cuda(), dirt.cuda()
    sg, sd = train_hip.scale(gd), train_hip.scale(dd)
    need = ctypes.c_int64()
    _lib.check(L.nic_conv_wgrad_work(c.n, c.uh, c.uw, c.kh, c.kw, c.ca, c.cb, ctypes.byref(need)), "nic_conv_wgrad_work")
    # the partials too: the kernel's stores go to `work`, the reduction's to dw
    wbuf, work = _banded(need.value)
    numel = c.kh * c.kw * c.ca * c.cb
    buf, dw = _banded(numel)
    _lib.check(L.nic_conv_wgrad(gd.data_ptr(), c.n, c.gat_hw[0], c.gat_hw[1], c.ca, dd.data_ptr(), c.uh, c.uw, c.cb, c.kh,
                                c.kw, c.stride, c.pad[0], c.pad[1], sg.data_ptr(), sd.data_ptr(), dw.data_ptr(),
                                work.data_ptr(), need.value, torch.cuda.current_stream().cuda_stream), "nic_conv_wgrad")
    torch.cuda.synchronize()
    _check_bands(buf, numel, "w6 dw")
    _check_bands(wbuf, need.value, "w6 work")
    assert _rel_err(dw.view(c.kh, c.kw, c.ca, c.cb), ref) <= TOL
