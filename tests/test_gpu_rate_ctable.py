"""The context rate loss on the GPU: nic_rate_ctable / nic_rate_ctable_grad against the float64
reference (tests/rate_ctable_ref.py), against the static pair, against the container's own counting
kernel, Training(rate="context") on the HIP backend against the torch backend, and the exported
context prior in the .nic version 3 coder.

The yardstick is that of tests/test_gpu_rate_table.py: on the same inputs (one fp32 table L on every
side) the fp32 PyTorch restatement (training.context_bits on the device) has an error e32 against
the float64 reference; the HIP error may be at most 2 e32 + EPS x the sum of the absolute terms
(per plane for the bits; for dL per (row, context) row, the largest entry's).  dy is elementwise:
the kernel and the formula (255 g) (L[x][k+1] - L[x][k]) evaluated in fp32 by PyTorch do the same
arithmetic, 1 ulp.

Measured on the MI355X (pytest -s prints them), worst case over the shapes, error / yardstick:
see DESIGN section 22.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import prior as P  # noqa: E402
from neural_network_image_compression_amd import train_hip  # noqa: E402
from neural_network_image_compression_amd import training as T  # noqa: E402
from tests import rate_ctable_ref as RC  # noqa: E402
from tests.rate_gpu_common import G_KINDS, g as _g, nchw as _nchw, report, ulps as _ulps  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
CASES = [(shape, seg) for shape in RC.SHAPES for seg in RC.segs(shape)]
_report = functools.partial(report, "rate-ctable")


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """Host inputs of one shape and the same on the device: y, yc (NHWC), anchors, L (fp32, shared by
    every side)."""
    y, yc, anchors, logits = RC.case(shape)
    L = T.context_code_lengths(torch.from_numpy(logits)).numpy()
    dev = tuple(torch.from_numpy(t).cuda() for t in (y, yc, anchors, L))
    return (y, yc, anchors, L), dev


@functools.lru_cache(maxsize=None)
def _ref(shape, seg):
    """The float64 references of one case, computed once: bits and per g kind the gradients."""
    (y, yc, anchors, L), _ = _inputs(shape)
    m, groups = shape[0], shape[4]
    bits, bits_abs = RC.rate_ctable(y, L, anchors, groups, seg, yc)
    grads = {kind: RC.rate_ctable_grad(y, L, anchors, _g(kind, m, groups), groups, seg, yc) for kind in G_KINDS}
    return bits, bits_abs, grads


@pytest.mark.parametrize("shape,seg", CASES, ids=str)
def test_forward_matches_float64(shape, seg):
    m, h, w, c, groups = shape
    _, (yd, ycd, ad, Ld) = _inputs(shape)
    ref, ref_abs, _ = _ref(shape, seg)
    got = train_hip.rate_ctable(yd, Ld, ad, groups, seg, ycd)
    assert got.shape == (m,) and got.dtype == torch.float32
    e32 = np.abs(T.context_bits(_nchw(yd), Ld, ad, groups, seg, _nchw(ycd)).double().cpu().numpy() - ref)
    err = np.abs(got.double().cpu().numpy() - ref)
    _report(f"forward {shape} seg {seg}", float((err / ref_abs).max()), float((e32 / ref_abs).max()))
    assert np.all(err <= 2 * e32 + EPS * ref_abs)
    assert torch.equal(train_hip.rate_ctable(yd, Ld, ad, groups, seg, ycd), got)  # deterministic
    assert torch.equal(train_hip.rate_ctable_bits(yd, Ld, ad, groups, seg, ycd), got)


@pytest.mark.parametrize("shape,seg", CASES, ids=str)
def test_backward_matches_float64(shape, seg):
    m, h, w, c, groups = shape
    (y, yc, anchors, L), (yd, ycd, ad, Ld) = _inputs(shape)
    k, _ = RC.R.elements(y)
    x = RC.contexts(yc, anchors, groups, seg)
    rows = np.broadcast_to(RC.R.rows_of(m, c, groups), k.shape)
    rt, xt, kt = (torch.from_numpy(np.array(t)).cuda() for t in (rows, x, k))
    for kind in G_KINDS:
        dy_ref, dl_ref, dl_abs = _ref(shape, seg)[2][kind]
        g = _g(kind, m, groups)
        gd = torch.from_numpy(g).cuda()
        dy, dl = train_hip.rate_ctable_grad(yd, Ld, ad, gd, groups, seg, ycd)
        assert dl.shape == Ld.shape
        # dy: the formula in fp32, the same arithmetic
        dy32 = (255 * gd)[:, None, None, None] * (Ld[rt, xt, kt + 1] - Ld[rt, xt, kt])
        assert _ulps(dy, dy32) <= 1
        # and against float64: a difference and two products, four roundings of at most |L0| + |L1|
        dy_abs = 255.0 * np.abs(g)[:, None, None, None] * (np.abs(L[rows, x, k]) + np.abs(L[rows, x, k + 1]))
        assert np.all(np.abs(dy.double().cpu().numpy() - dy_ref) <= 4 * 2.0 ** -24 * dy_abs)
        # the restatement through autograd, the yardstick of dL
        y32, L32 = _nchw(yd).requires_grad_(), Ld.clone().requires_grad_()
        (T.context_bits(y32, L32, ad, groups, seg, _nchw(ycd)) * gd).sum().backward()
        e32 = np.abs(L32.grad.double().cpu().numpy() - dl_ref).max(axis=2)  # per (row, context)
        err = np.abs(dl.double().cpu().numpy() - dl_ref).max(axis=2)
        mag = dl_abs.max(axis=2)
        _report(f"dL {shape} seg {seg} {kind}", float((err / np.maximum(mag, 1e-30)).max()),
                float((e32 / np.maximum(mag, 1e-30)).max()), "dy ulps", _ulps(dy, dy32))
        assert np.all(err <= 2 * e32 + EPS * mag)
        # each alone (the other pointer NULL) and a second run: the same bits
        dy1, none = train_hip.rate_ctable_grad(yd, Ld, ad, gd, groups, seg, ycd, want_dl=False)
        assert none is None and torch.equal(dy1, dy)
        none, dl1 = train_hip.rate_ctable_grad(yd, Ld, ad, gd, groups, seg, ycd, want_dy=False)
        assert none is None and torch.equal(dl1, dl)
        dy2, dl2 = train_hip.rate_ctable_grad(yd, Ld, ad, gd, groups, seg, ycd)
        assert torch.equal(dy2, dy) and torch.equal(dl2, dl)


@pytest.mark.parametrize("shape,seg", CASES, ids=str)
def test_equal_rows_give_the_static_bits_and_dy(shape, seg):
    m, h, w, c, groups = shape
    _, (yd, ycd, ad, _) = _inputs(shape)
    _, logits = RC.R.case(shape)
    L2 = T.table_code_lengths(torch.from_numpy(logits)).cuda()
    L3 = L2[:, None, :].expand(-1, 3, -1).contiguous()
    gd = torch.from_numpy(_g("signs", m, groups)).cuda()
    want_dy, want_dl = train_hip.rate_table_grad(yd, L2, gd, groups)
    for src in (ycd, None):
        assert torch.equal(train_hip.rate_ctable_bits(yd, L3, ad, groups, seg, src), train_hip.rate_table_bits(yd, L2, groups))
        dy, dl = train_hip.rate_ctable_grad(yd, L3, ad, gd, groups, seg, src)
        assert torch.equal(dy, want_dy)
        # the three context rows split the static row's terms
        assert np.abs((dl.double().sum(dim=1) - want_dl.double()).cpu().numpy()).max() <= \
            1e-5 * float(want_dl.abs().max())


@pytest.mark.parametrize("shape", RC.SHAPES, ids=str)
def test_no_yc_is_y_and_one_pixel_segments_are_static(shape):
    m, h, w, c, groups = shape
    _, (yd, ycd, ad, Ld) = _inputs(shape)
    gd = torch.from_numpy(_g("signs", m, groups)).cuda()
    for seg in RC.segs(shape):
        assert torch.equal(train_hip.rate_ctable_bits(yd, Ld, ad, groups, seg), train_hip.rate_ctable_bits(yd, Ld, ad, groups, seg, yd))
        a, b = train_hip.rate_ctable_grad(yd, Ld, ad, gd, groups, seg), train_hip.rate_ctable_grad(yd, Ld, ad, gd, groups, seg, yd)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # seg_pixels = 1: every element in context 0, a static call on the rows [:, 0, :]
    L0 = Ld[:, 0, :].contiguous()
    assert torch.equal(train_hip.rate_ctable_bits(yd, Ld, ad, groups, 1, ycd), train_hip.rate_table_bits(yd, L0, groups))
    dy, dl = train_hip.rate_ctable_grad(yd, Ld, ad, gd, groups, 1, ycd)
    dy0, dl0 = train_hip.rate_table_grad(yd, L0, gd, groups)
    assert torch.equal(dy, dy0) and torch.equal(dl[:, 0, :], dl0) and not bool(dl[:, 1:, :].any())


@pytest.mark.parametrize("seg", [32, 5])
def test_dl_counts_are_the_containers(golden, seg):
    """rint(dL) under g = 1 at y = z / 255 is Codec.cprior_count's device count: the container's own
    context rule, checked on the device."""
    from neural_network_image_compression_amd.codec import Codec

    z = golden("imagenet4_trained")["latent"]
    n = z.shape[0]
    codec = Codec(0)
    zd = torch.from_numpy(z).cuda()
    static = torch.zeros((96, 256), dtype=torch.int64, device="cuda")
    codec.prior_count(zd, static)
    anchors = static.argmax(dim=1).to(torch.uint8)
    counts = torch.zeros((96, 3, 256), dtype=torch.int64, device="cuda")
    codec.cprior_count(zd, anchors, counts, seg)
    yd = torch.from_numpy(RC.planes_of(z)).cuda()
    Ld = torch.zeros((96, 3, 256), device="cuda")
    _, dl = train_hip.rate_ctable_grad(yd, Ld, anchors, torch.ones(3 * n, device="cuda"), 3, seg, want_dy=False)
    assert int(counts.sum()) == z.size and torch.equal(torch.round(dl).long(), counts)


def test_edge_inputs_equal_the_clamped_inputs():
    y, yc, y_cl, yc_cl, anchors = RC.edge_case()
    _, (_, _, _, Ld) = _inputs((6, 5, 7, 32, 3))
    L = Ld.cpu().numpy()
    yd, ycd, ycl, yccl = (torch.from_numpy(t).cuda() for t in (y, yc, y_cl, yc_cl))
    ad = torch.from_numpy(anchors).cuda()
    g = torch.full((3,), 1.0 / 64, device="cuda")
    for seg in (5, 32):
        ref, ref_abs = RC.rate_ctable(y, L, anchors, 3, seg, yc)
        got = train_hip.rate_ctable_bits(yd, Ld, ad, 3, seg, ycd)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, train_hip.rate_ctable_bits(ycl, Ld, ad, 3, seg, yccl))
        e32 = np.abs(T.context_bits(_nchw(ycl), Ld, ad, 3, seg, _nchw(yccl)).double().cpu().numpy() - ref)
        err = np.abs(got.double().cpu().numpy() - ref)
        assert np.all(np.isfinite(err)) and np.all(err <= 2 * e32 + EPS * ref_abs)
        dy, dl = train_hip.rate_ctable_grad(yd, Ld, ad, g, 3, seg, ycd)
        assert bool(torch.isfinite(dy).all()) and bool(torch.isfinite(dl).all())
        dy_cl, dl_cl = train_hip.rate_ctable_grad(ycl, Ld, ad, g, 3, seg, yccl)
        assert torch.equal(dy, dy_cl) and torch.equal(dl, dl_cl)
        want = RC.rate_ctable_grad(y, L, anchors, np.full(3, 1.0 / 64), 3, seg, yc)[1]
        assert np.abs(dl.double().cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("shape", [(6, 5, 7, 32, 3), (15, 16, 16, 32, 3)], ids=str)
def test_plane_0_does_not_depend_on_what_lies_before_it(shape):
    """Plane 0 of a tensor that starts its allocation gives what the same plane gives inside a larger
    batch (where other planes precede it): no left read crosses the plane start."""
    m, h, w, c, groups = shape
    _, (yd, ycd, ad, Ld) = _inputs(shape)
    La, aa = Ld[:c].contiguous(), ad[:c].contiguous()  # group 0's rows
    big_y = torch.cat([torch.rand_like(yd[:1]), yd[:1]]).contiguous()  # the plane behind another one
    big_c = torch.cat([torch.rand_like(ycd[:1]), ycd[:1]]).contiguous()
    one_y, one_c = yd[:1].clone(), ycd[:1].clone()  # the plane at the start of its own allocation
    g1, g2 = torch.tensor([0.5], device="cuda"), torch.tensor([0.0, 0.5], device="cuda")
    for seg in RC.segs(shape):
        alone = train_hip.rate_ctable_bits(one_y, La, aa, 1, seg, one_c)
        assert torch.equal(alone, train_hip.rate_ctable_bits(big_y, La, aa, 1, seg, big_c)[1:])
        assert torch.equal(alone, train_hip.rate_ctable_bits(yd, Ld, ad, groups, seg, ycd)[:1])
        dy, dl = train_hip.rate_ctable_grad(one_y, La, aa, g1, 1, seg, one_c)
        dy2, dl2 = train_hip.rate_ctable_grad(big_y, La, aa, g2, 1, seg, big_c)
        assert torch.equal(dy, dy2[1:]) and not bool(dy2[:1].any())
        assert float((dl - dl2).abs().max()) <= 1e-5 * float(dl.abs().max())  # (other slabs: another order)


def test_autograd_function_honours_needs_input_grad(monkeypatch):
    shape, seg = (6, 5, 7, 32, 3), 5
    (y, yc, anchors, L), (yd0, ycd, ad, Ld0) = _inputs(shape)
    g = torch.from_numpy(_g("signs", 6, 3)).cuda()
    seen = []
    real = train_hip.rate_ctable_grad

    def spy(y, L, anchors, g, groups, seg_pixels, yc=None, want_dy=True, want_dl=True):
        seen.append((bool(want_dy), bool(want_dl)))
        return real(y, L, anchors, g, groups, seg_pixels, yc, want_dy, want_dl)

    monkeypatch.setattr(train_hip, "rate_ctable_grad", spy)
    yd, Ld = yd0.clone().requires_grad_(), Ld0.clone().requires_grad_()
    ycg = ycd.clone().requires_grad_()
    (train_hip.rate_ctable(yd, Ld.detach(), ad, 3, seg, ycg) * g).sum().backward()
    (train_hip.rate_ctable(yd.detach(), Ld, ad, 3, seg, ycg) * g).sum().backward()
    assert seen == [(True, False), (False, True)]
    assert ycg.grad is None  # never a gradient for yc
    dy_ref, dl_ref, _ = _ref(shape, seg)[2]["signs"]
    assert np.abs(yd.grad.double().cpu().numpy() - dy_ref).max() <= 1e-5 * np.abs(dy_ref).max()
    assert np.abs(Ld.grad.double().cpu().numpy() - dl_ref).max() <= 1e-5 * np.abs(dl_ref).max()
    # through the public function, from logits
    _, _, _, logits = RC.case(shape)
    z = torch.from_numpy(logits).cuda().requires_grad_()
    T.context_rate(yd.detach(), z, ad, 3, seg, ycd, hip=True).sum().backward()
    zc = torch.from_numpy(logits).requires_grad_()
    T.context_rate(_nchw(yd.detach()).cpu(), zc, ad.cpu(), 3, seg, _nchw(ycd).cpu()).sum().backward()
    assert float((z.grad.cpu() - zc.grad).abs().max()) <= 1e-4 * float(zc.grad.abs().max())


def test_empty_batch_and_wrong_arguments():
    Ld = torch.zeros((96, 3, 256), device="cuda")
    ad = torch.zeros(96, dtype=torch.uint8, device="cuda")
    y0 = torch.zeros((0, 4, 4, 32), device="cuda")
    assert train_hip.rate_ctable(y0, Ld, ad, 3, 32).shape == (0,)
    dy, dl = train_hip.rate_ctable_grad(y0, torch.ones_like(Ld), ad, torch.zeros((0,), device="cuda"), 3, 32)
    assert dy.shape == y0.shape and dl.shape == Ld.shape and not bool(dl.any())
    y3 = torch.zeros((3, 4, 4, 32), device="cuda")
    for bad in (lambda: train_hip.rate_ctable(y3, Ld[:64], ad, 3, 32),  # a short table
                lambda: train_hip.rate_ctable(y3, Ld[:, 0], ad, 3, 32),  # a static table
                lambda: train_hip.rate_ctable(y3, Ld, ad[:32], 3, 32),  # one group's anchors
                lambda: train_hip.rate_ctable(y3, Ld, ad.int(), 3, 32),  # not bytes
                lambda: train_hip.rate_ctable(y3, Ld, ad, 3, 0),  # seg_pixels = 0
                lambda: train_hip.rate_ctable_grad(y3, Ld, ad, torch.zeros(3, device="cuda"), 3, 0),
                lambda: train_hip.rate_ctable(y3, Ld, ad, 3, 32, y3[:, :2]),  # another yc
                lambda: train_hip.rate_ctable(torch.zeros((4, 4, 4, 32), device="cuda"), Ld, ad, 3, 32)):
        with pytest.raises(ValueError):
            bad()


def test_training_step_hip_matches_torch_backend(tmp_path):
    from neural_network_image_compression_amd import weights as W

    w0 = W.seeded_weights(0, init="glorot")
    imgs = torch.randint(0, 256, (4, 32, 32, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    anchors = np.random.default_rng(9).integers(0, 6, 96)
    out = {}
    for be in ("hip", "torch"):
        tr = T.Training(device="cuda", weights=w0, seed=0, checkpoint_dir=str(tmp_path) + "/", backend=be,
                        rate="context", anchors=anchors, seg_pixels=5)
        out[be] = ([tr.train_step(imgs, 0.01) for _ in range(2)], tr.table_logits.detach().cpu(),
                   tr.ctx_logits.detach().cpu())
        assert tr.entropy_model is None
    for mh, mt in zip(out["hip"][0], out["torch"][0]):
        assert set(mh) == set(mt)
        for key in mh:
            for a, b in zip(np.ravel(mh[key]), np.ravel(mt[key])):
                assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (key, a, b)
    for i in (1, 2):
        a, b = out["hip"][i], out["torch"][i]
        assert bool(((a - b).abs() <= 1e-4 * b.abs().clamp_min(1.0)).all()), float((a - b).abs().max())
        assert bool(b.any())  # the table moved


def test_exported_context_prior_reaches_the_container(tmp_path):
    from neural_network_image_compression_amd.codec import Codec

    tr = T.Training(device="cuda", seed=0, checkpoint_dir=str(tmp_path) + "/", rate="context")
    imgs = torch.randint(0, 256, (4, 32, 32, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    for _ in range(3):
        tr.train_step(imgs, 0.01)
    tr.refresh_anchors()
    cp = tr.context_prior()
    codec = Codec(0)
    codec.set_context_prior(cp)
    z = torch.randint(0, 256, (1, 8, 8, 96), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    buf, sizes = codec.rans3_encode(z)
    assert torch.equal(codec.rans3_decode(buf, sizes, 8, 8), z)
    # the device's normalisation of the same pseudo-counts
    logits = tr.ctx_logits.detach().cpu().numpy().astype(np.float64)
    e = np.exp(logits - logits.max(axis=2, keepdims=True))
    counts = torch.from_numpy(P.context_pseudo_counts(e / e.sum(axis=2, keepdims=True))).cuda()
    assert np.array_equal(codec.cprior_build(counts).cpu().numpy(), cp.freqs)
    assert np.array_equal(cp.anchors, np.argmax(tr.table_logits.detach().cpu().numpy(), axis=1))
    tr._save()
    assert P.ContextPrior.load(str(tmp_path / "prior.nicc")) == cp
    assert P.Prior.load(str(tmp_path / "prior.nicp")) == tr.prior()
