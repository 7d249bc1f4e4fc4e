"""The context rate loss without a GPU: training.context_rate (the PyTorch restatement) against the
float64 reference (tests/rate_ctable_ref.py) and against the version-3 container's own context rule
(tests/rans3_ref.py), prior.context_from_probabilities, Training(rate="context") on the CPU, and
the C entry points' argument checks.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from neural_network_image_compression_amd import _lib
from neural_network_image_compression_amd import bitstream
from neural_network_image_compression_amd import prior as P
from neural_network_image_compression_amd import training as T
from tests import rans2_ref
from tests import rans3_ref as R3
from tests import rate_ctable_ref as RC

CASES = [(shape, seg) for shape in RC.SHAPES for seg in RC.segs(shape)]


def _nchw(y):
    return torch.from_numpy(np.ascontiguousarray(y.transpose(0, 3, 1, 2)))


@functools.lru_cache(maxsize=None)
def _case(shape):
    y, yc, anchors, logits = RC.case(shape)
    return y, yc, anchors, T.context_code_lengths(torch.from_numpy(logits)).numpy()  # one fp32 L on every side


@pytest.mark.parametrize("shape", [s for s in RC.SHAPES if s[1] * s[2] >= 9], ids=str)
def test_case_generator_reaches_every_context(shape):
    RC.assert_contexts_occur(shape)


@pytest.mark.parametrize("shape,seg", CASES, ids=str)
def test_context_bits_matches_float64(shape, seg):
    m, h, w, c, groups = shape
    y, yc, anchors, L = _case(shape)
    g = np.random.default_rng(m).standard_normal(m).astype(np.float32)
    ref, _ = RC.rate_ctable(y, L, anchors, groups, seg, yc)
    dy_ref, dl_ref, _ = RC.rate_ctable_grad(y, L, anchors, g, groups, seg, yc)
    yt, Lt, yct = _nchw(y).requires_grad_(), torch.from_numpy(L).requires_grad_(), _nchw(yc).requires_grad_()
    bits = T.context_bits(yt, Lt, torch.from_numpy(anchors), groups, seg, yct)
    assert bits.shape == (m,) and bits.dtype == torch.float32
    (bits * torch.from_numpy(g)).sum().backward()
    assert yct.grad is None  # the context is computed under no_grad
    assert np.all(np.abs(bits.detach().numpy() - ref) <= 1e-5 * np.abs(ref))
    assert np.abs(yt.grad.numpy().transpose(0, 2, 3, 1) - dy_ref).max() <= 1e-5 * np.abs(dy_ref).max()
    assert np.abs(Lt.grad.numpy() - dl_ref).max() <= 1e-5 * np.abs(dl_ref).max()
    # yc = None reads the contexts from y itself
    none = T.context_bits(_nchw(y), torch.from_numpy(L), torch.from_numpy(anchors), groups, seg)
    same = T.context_bits(_nchw(y), torch.from_numpy(L), torch.from_numpy(anchors), groups, seg, _nchw(y))
    assert torch.equal(none, same)
    want = RC.rate_ctable(y, L, anchors, groups, seg)[0]
    assert np.all(np.abs(none.numpy() - want) <= 1e-5 * np.abs(want))


def test_context_rate_through_logits():
    shape, seg = (6, 5, 7, 32, 3), 5
    m, h, w, c, groups = shape
    y, yc, anchors, logits = RC.case(shape, seed=1)
    L = RC.code_lengths(logits)
    ref, _ = RC.rate_ctable(y, L, anchors, groups, seg, yc)
    _, dl_ref, _ = RC.rate_ctable_grad(y, L, anchors, np.ones(m), groups, seg, yc)
    p = np.exp(-L * np.log(2.0))
    dz_ref = -(dl_ref - p * dl_ref.sum(axis=2, keepdims=True)) / np.log(2.0)
    zt = torch.from_numpy(logits).requires_grad_()
    bits = T.context_rate(_nchw(y), zt, torch.from_numpy(anchors), groups, seg, _nchw(yc))
    bits.sum().backward()
    assert np.all(np.abs(bits.detach().numpy() - ref) <= 1e-5 * np.abs(ref))
    assert np.abs(zt.grad.numpy() - dz_ref).max() <= 1e-4 * np.abs(dz_ref).max()
    zero = T.context_rate(_nchw(y), torch.zeros((groups * c, 3, 256)), torch.from_numpy(anchors), groups, seg)
    assert torch.equal(zero, torch.full((m,), 8.0 * h * w * c))


@pytest.mark.parametrize("shape,seg", CASES, ids=str)
def test_equal_rows_give_the_table_rate(shape, seg):
    m, h, w, c, groups = shape
    y, yc, anchors, _ = _case(shape)
    _, logits = RC.R.case(shape)
    L2 = T.table_code_lengths(torch.from_numpy(logits))
    L3 = L2[:, None, :].expand(-1, 3, -1).contiguous()
    got = T.context_bits(_nchw(y), L3, torch.from_numpy(anchors), groups, seg, _nchw(yc))
    assert torch.equal(got, T.table_bits(_nchw(y), L2, groups))


def test_edge_inputs_are_clamped():
    y, yc, y_cl, yc_cl, anchors = RC.edge_case()
    _, _, _, L = _case((6, 5, 7, 32, 3))
    a, Lt = torch.from_numpy(anchors), torch.from_numpy(L)
    for seg in (5, 32):
        got = T.context_bits(_nchw(y), Lt, a, 3, seg, _nchw(yc))
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, T.context_bits(_nchw(y_cl), Lt, a, 3, seg, _nchw(yc_cl)))
        ref = RC.rate_ctable(y, L, anchors, 3, seg, yc)[0]
        assert np.array_equal(ref, RC.rate_ctable(y_cl, L, anchors, 3, seg, yc_cl)[0])
        assert np.all(np.abs(got.numpy() - ref) <= 1e-5 * np.abs(ref))


def test_context_bits_rejects_bad_arguments():
    y, a = torch.zeros((3, 32, 2, 2)), torch.zeros(96, dtype=torch.uint8)
    L = torch.zeros((96, 3, 256))
    T.context_bits(y, L, a, 3)
    for bad in (lambda: T.context_bits(y, L[:64], a, 3), lambda: T.context_bits(y, L[:, 0], a, 3),
                lambda: T.context_bits(y, L, a[:32], 3), lambda: T.context_bits(y, L, a.long(), 3),
                lambda: T.context_bits(y, L, a, 3, seg_pixels=0), lambda: T.context_bits(y, L, a, 2),
                lambda: T.context_bits(y, L, a, 3, yc=y[:, :, :1])):
        with pytest.raises(ValueError):
            bad()


# ---- against the version-3 container's own rule (the trained golden latents) -----------------------
@pytest.fixture(scope="module")
def latents(golden):
    return golden("imagenet4_trained")["latent"]


@pytest.mark.parametrize("seg", [32, 5])
def test_context_rule_is_the_containers(latents, seg):
    n = latents.shape[0]
    static = rans2_ref.fit_prior(list(latents))
    anchors = np.array(R3.anchors_of(static), np.uint8)
    y = RC.planes_of(latents)
    # the context of every byte
    x = RC.contexts(y, anchors, 3, seg)  # (3 N, h, w, 32)
    for i, z in enumerate(latents):
        want = R3.contexts_of(z, anchors, seg).reshape(*z.shape)
        got = np.concatenate([x[g * n + i] for g in range(3)], axis=-1)
        assert np.array_equal(got, want)
    # and the counts: dL under g = 1 at y = z / 255
    want = R3.counts_of(latents, anchors, seg)
    dl_ref = RC.rate_ctable_grad(y, np.zeros((96, 3, 256)), anchors, np.ones(3 * n), 3, seg)[1]
    assert np.array_equal(np.rint(dl_ref).astype(np.int64), want)
    Lt = torch.zeros((96, 3, 256), requires_grad=True)
    T.context_bits(_nchw(y), Lt, torch.from_numpy(anchors), 3, seg).sum().backward()
    assert np.array_equal(np.rint(Lt.grad.numpy()).astype(np.int64), want)


@pytest.mark.parametrize("seg", [32, 5])
def test_conditioning_pays(latents, seg):
    """Under the latents' own empirical frequencies the context code length is no more than the
    static one (conditioning cannot raise an empirical entropy); zero counts are floored so that no
    length is infinite (those symbols do not occur)."""
    n = latents.shape[0]
    anchors = np.array(R3.anchors_of(rans2_ref.fit_prior(list(latents))), np.uint8)
    cc = R3.counts_of(latents, anchors, seg).astype(np.float64)  # (96, 3, 256)
    sc = cc.sum(axis=1)
    L3 = -np.log2(np.maximum(cc, 1e-3) / np.maximum(cc.sum(axis=2, keepdims=True), 1.0))
    L2 = -np.log2(np.maximum(sc, 1e-3) / sc.sum(axis=1, keepdims=True))
    y = _nchw(RC.planes_of(latents))
    ctx = T.context_bits(y, torch.from_numpy(L3.astype(np.float32)), torch.from_numpy(anchors), 3, seg)
    static = T.table_bits(y, torch.from_numpy(L2.astype(np.float32)), 3)
    c_bits, s_bits = float(ctx.double().sum()), float(static.double().sum())
    print(f"\n[rate-ctable] seg {seg}: context {c_bits:.0f} bits, static {s_bits:.0f} bits ({c_bits / s_bits:.3f})")
    assert c_bits <= s_bits


# ---- prior.context_from_probabilities ----------------------------------------------------------------
def test_context_from_probabilities(tmp_path):
    rng = np.random.default_rng(13)
    z = 3.0 * rng.standard_normal((96, 3, 256))
    z[5, 1] = 0.0  # a uniform row
    z[7, 2, 9] = 60.0  # a peaked one
    e = np.exp(z - z.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    anchors = rng.integers(0, 256, 96)
    cp = P.context_from_probabilities(anchors, p)
    assert isinstance(cp, P.ContextPrior) and np.array_equal(cp.anchors, anchors)
    assert cp.freqs.min() >= 1 and cp.freqs.max() <= 4096 and np.all(cp.freqs.sum(axis=2) == 4096)
    assert np.all(cp.freqs[5, 1] == 16)
    counts = P.context_pseudo_counts(p)
    assert np.array_equal(counts, np.rint(p * 2.0 ** 40).astype(np.int64))
    want = np.array(R3.normalise_counts(counts))
    assert np.array_equal(cp.freqs, want)
    for ch in (0, 40, 95):  # per row it is from_probabilities' rule
        for x in range(3):
            assert np.array_equal(P.from_probabilities(np.broadcast_to(p[ch, x], (96, 256))).freqs[0], cp.freqs[ch, x])
    R3.check_prior((cp.anchors.tolist(), cp.freqs.tolist()))
    assert cp.id == R3.prior_id((cp.anchors.tolist(), cp.freqs))
    path = tmp_path / "t.nicc"
    cp.save(str(path))
    assert P.ContextPrior.load(str(path)) == cp and P.ContextPrior.from_bytes(cp.to_bytes()) == cp
    assert path.read_bytes() == R3.write_nicc((cp.anchors.tolist(), cp.freqs.astype(int).tolist()))
    with pytest.raises(ValueError):
        P.context_from_probabilities(anchors, p[:, 0])
    with pytest.raises(ValueError):
        P.context_from_probabilities(anchors, 2 * p)


# ---- Training(rate="context") on the CPU ---------------------------------------------------------------
def _no_png(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the PNG target was reached")

    monkeypatch.setattr(bitstream, "png_sizes", boom)
    monkeypatch.setattr(T, "png_sizes", boom)
    monkeypatch.setattr(T, "png_bpp_planes", boom)


def test_training_with_context_rate_on_cpu(tmp_path, monkeypatch):
    _no_png(monkeypatch)
    tr = T.Training(device="cpu", seed=0, checkpoint_dir=str(tmp_path) + "/", rate="context")
    assert tuple(tr.table_logits.shape) == (96, 256) and not bool(tr.table_logits.any())
    assert tuple(tr.ctx_logits.shape) == (96, 3, 256) and not bool(tr.ctx_logits.any())
    assert tr.anchors.dtype == torch.uint8 and not bool(tr.anchors.any()) and tr.seg_pixels == 32
    batch = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (4, 32, 32, 3), dtype=np.uint8))
    first = tr.train_step(batch, 0.01, flip=False)
    assert tr.entropy_model is None
    assert set(first) == {"ssim", "bpp", "entropy_loss", "loss"}
    assert np.abs(np.array(first["bpp"]) - 4.0).max() <= 1e-5  # 8 bits x 32 channels / 64 pixels
    assert abs(first["entropy_loss"] - 4.0) <= 1e-5  # the context term alone
    second = tr.train_step(batch, 0.01, flip=False)
    assert second["entropy_loss"] < first["entropy_loss"]
    assert bool(tr.table_logits.any()) and bool(tr.ctx_logits.any())  # one Adam moved both tables
    # refresh_anchors: the static table's argmax, the lowest symbol on ties
    with torch.no_grad():
        tr.table_logits[3, 200] = 9.0
        tr.table_logits[4, 17] = tr.table_logits[4, 90] = 8.0
    tr.refresh_anchors()
    want = np.argmax(tr.table_logits.detach().numpy(), axis=1)
    assert int(tr.anchors[3]) == 200 and int(tr.anchors[4]) == 17 and np.array_equal(tr.anchors.numpy(), want)
    cp, pr = tr.context_prior(), tr.prior()
    assert isinstance(cp, P.ContextPrior) and isinstance(pr, P.Prior) and np.array_equal(cp.anchors, want)
    tr._save()
    assert P.Prior.load(str(tmp_path / "prior.nicp")) == pr
    assert P.ContextPrior.load(str(tmp_path / "prior.nicc")) == cp


def test_training_call_refreshes_anchors_each_epoch(tmp_path, monkeypatch):
    _no_png(monkeypatch)
    tr = T.Training(device="cpu", seed=0, checkpoint_dir=str(tmp_path) + "/", rate="context")
    calls = []
    real = tr.refresh_anchors
    monkeypatch.setattr(tr, "refresh_anchors", lambda: (calls.append(tr.epoch), real())[1])
    x = np.random.default_rng(2).integers(0, 256, (2, 16, 16, 3), dtype=np.uint8)
    tr(x, None, 2, 2, 0.01, verbose=False)
    assert calls == [0, 1]


def test_given_anchors_stay_put(tmp_path):
    given = np.arange(96) + 100
    tr = T.Training(device="cpu", rate="context", anchors=given, seg_pixels=5, checkpoint_dir=str(tmp_path) + "/")
    assert tr.seg_pixels == 5 and np.array_equal(tr.anchors.numpy(), given)
    with torch.no_grad():
        tr.table_logits[:, 3] = 5.0
    tr.refresh_anchors()
    assert np.array_equal(tr.anchors.numpy(), given)
    # a Prior gives its rows' argmax, a ContextPrior its anchors
    rng = np.random.default_rng(3)
    p = rng.random((96, 256)) + 1e-3
    pr = P.from_probabilities(p / p.sum(axis=1, keepdims=True))
    assert np.array_equal(T.Training(device="cpu", rate="context", anchors=pr).anchors.numpy(), P.anchors_of(pr))
    cp = P.ContextPrior(given, np.full((96, 3, 256), 16))
    assert np.array_equal(T.Training(device="cpu", rate="context", anchors=cp).anchors.numpy(), given)
    for bad in (np.arange(95), np.full(96, 256), np.full(96, 0.5)):
        with pytest.raises(ValueError):
            T.Training(device="cpu", rate="context", anchors=bad)
    with pytest.raises(ValueError):
        T.Training(device="cpu", rate="context", seg_pixels=0)


def test_rate_argument_names_every_legal_value():
    with pytest.raises(ValueError) as e:
        T.Training(device="cpu", rate="zip")
    for name in ("png", "table", "context"):
        assert repr(name) in str(e.value)
    tr = T.Training(device="cpu", rate="table")
    assert tr.ctx_logits is None and tr.anchors is None
    with pytest.raises(ValueError):
        tr.context_prior()
    tr.refresh_anchors()  # nothing to do


# ---- the C entry points' argument checks ---------------------------------------------------------------
def test_rate_ctable_capi_rejects_without_a_gpu():
    L = _lib.lib()
    E, S, OK = _lib.NIC_EINVAL, _lib.NIC_ESHAPE, _lib.NIC_OK
    assert L.nic_version() >= 1400
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # never dereferenced: every call below fails its checks first
    f = ctypes.c_int64()
    # the documented count: max(m ceil(h w c / 1024), 3 groups ceil((m / groups) h w / 128) c 256)
    assert L.nic_rate_ctable_work(192, 16, 16, 32, 3, ctypes.byref(f)) == OK and f.value == 3 * 3 * 128 * 32 * 256
    assert L.nic_rate_ctable_work(6, 5, 7, 32, 3, ctypes.byref(f)) == OK and f.value == 3 * 3 * 1 * 32 * 256
    assert L.nic_rate_ctable_work(1, 300, 300, 1, 1, ctypes.byref(f)) == OK and f.value == 3 * 704 * 256
    assert L.nic_rate_ctable_work(0, 4, 4, 32, 3, ctypes.byref(f)) == OK and f.value == 0
    assert L.nic_rate_ctable_work(3, 4, 4, 32, 3, None) == E

    def fwd(y=p, yc=p, tab=p, a=p, m=3, h=4, w=4, ch=32, groups=3, seg=32, out=p, work=p, n=1 << 30):
        return L.nic_rate_ctable(y, yc, tab, a, m, h, w, ch, groups, seg, out, work, n, None)

    def bwd(y=p, yc=p, tab=p, a=p, g=p, m=3, h=4, w=4, ch=32, groups=3, seg=32, dy=p, dl=p, work=p, n=1 << 30):
        return L.nic_rate_ctable_grad(y, yc, tab, a, g, m, h, w, ch, groups, seg, dy, dl, work, n, None)

    for ch in (0, 65):
        assert L.nic_rate_ctable_work(3, 4, 4, ch, 3, ctypes.byref(f)) == S
        assert fwd(ch=ch) == S and bwd(ch=ch) == S
    assert fwd(m=4) == S and bwd(m=4) == S and fwd(groups=0) == S and bwd(h=0) == S
    assert fwd(h=1 << 14, w=1 << 14) == S
    for seg in (0, -1):
        assert fwd(seg=seg) == E and bwd(seg=seg) == E
    for kw in ({"y": None}, {"tab": None}, {"a": None}, {"out": None}, {"work": None}):
        assert fwd(**kw) == E
    for kw in ({"y": None}, {"tab": None}, {"a": None}, {"g": None}, {"work": None}, {"dy": None, "dl": None}):
        assert bwd(**kw) == E
    assert bwd(m=0, dy=None, dl=None) == E
    need = 3 * 3 * 1 * 32 * 256
    assert fwd(n=need - 1) == E and bwd(n=need - 1) == E
    # an empty batch is OK (nothing is read or written without dL)
    assert L.nic_rate_ctable(None, None, None, None, 0, 4, 4, 32, 3, 32, None, None, 0, None) == OK
    assert L.nic_rate_ctable_grad(None, None, None, None, None, 0, 4, 4, 32, 3, 32, p, None, None, 0, None) == OK
