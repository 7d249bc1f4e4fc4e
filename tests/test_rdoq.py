"""CPU checks of rate-distortion optimised quantisation: the NumPy reference
(tests/rdoq_ref.py) on the golden latents -- lambda 0 is the identity, the trellis against an
exhaustive search over every choice of short chains, the priced cost of every chain, real file sizes
through rans2_ref / rans3_ref and their round trips -- and the checks nic_rdoq and the directory
driver make before any GPU call."""
import itertools

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from neural_network_image_compression_amd import bitstream as B
from tests import rans2_ref as R2
from tests import rans3_ref as R3
from tests import rdoq_ref as Q
from tests.conftest import load_case

CASES = ("kodim21_256_trained", "imagenet4_trained", "odd37x53")
LAMS = (0.01, 0.1, 1.0, 16.0)
SEG_PIXELS = (1, 5, 32, 64)


@pytest.fixture(scope="module")
def cases():
    return {name: load_case(name) for name in CASES}


@pytest.fixture(scope="module")
def priors(cases):
    """The static prior fitted on the four imagenet4_trained latents and the context prior fitted on
    them with its anchors."""
    latents = list(cases["imagenet4_trained"]["latent"])
    static = R2.fit_prior(latents)
    return static, R3.fit_context_prior(latents, static)


def _chain_costs(zq, f, cprior, lam_fix, seg_pixels):
    """Priced cost of every (segment, channel) chain of one image: (nseg, 96) int64."""
    anchors, freqs = cprior
    q = np.asarray(zq).reshape(-1, Q.CH).astype(np.int64)
    d = np.asarray(f, np.float32).reshape(-1, Q.CH) * np.float32(255.0) - q.astype(np.float32)
    J = (np.rint(d * d * np.float32(65536.0)).astype(np.int64) << 16) + lam_fix * Q.COST16[np.asarray(freqs, np.int64)][
        np.arange(Q.CH)[None], R3.contexts_of(zq, anchors, seg_pixels), q]
    return np.add.reduceat(J, np.arange(0, len(J), seg_pixels), axis=0)


@pytest.mark.parametrize("case", CASES)
def test_lambda_zero_returns_the_input(cases, priors, case):
    static, cprior = priors
    z, f = cases[case]["latent"], cases[case]["prequant"]
    np.testing.assert_array_equal(Q.rdoq_static(z, f, static, 0), z)
    for sp in SEG_PIXELS:
        np.testing.assert_array_equal(Q.rdoq_context(z, f, cprior, 0, sp), z)


def _exhaustive(cand, D, cost_rows, anchor, lam_fix):
    """The cheapest of all 2^L choices; among equals the tie rule's: state 0 at the last pixel if any
    optimum ends there, then likewise backwards -- the least choice read from the end."""
    best = None
    for choice in itertools.product((0, 1), repeat=len(cand)):
        key = (Q.chain_cost(choice, cand, D, cost_rows, anchor, lam_fix), choice[::-1])
        if best is None or key < best:
            best = key
    return list(best[1][::-1]), best[0]


def _fixture_chains(cases, cprior):
    """Chains of length 1..10 from the three fixtures: for every length, the four channels whose codes
    vary most and the four whose pre-quant values lie closest to a rounding boundary."""
    anchors, freqs = cprior
    cost = Q.COST16[np.asarray(freqs, np.int64)]
    for name in CASES:
        z, f = cases[name]["latent"][0].reshape(-1, Q.CH), cases[name]["prequant"][0].reshape(-1, Q.CH)
        cand, D = Q.candidates(z, f)
        frac = np.abs(np.abs(f * np.float32(255.0) - z) - 0.5).mean(0)
        chans = sorted(set(np.argsort(-z.std(0))[:4].tolist() + np.argsort(frac)[:4].tolist()))
        for n in range(1, 11):
            for c in chans:
                at = (7 * n + c) % (len(z) - n + 1)
                yield f"{name} c{c} p{at}+{n}", cand[at:at + n, c], D[at:at + n, c], cost[c], int(anchors[c])


def _random_chains():
    """Seeded chains: skewed rows, anchors at 0, 255 and in between, codes at and around the anchor and at
    the ends of the range, pre-quant values anywhere in the code's rounding interval and on its edges."""
    rng = np.random.default_rng(25)
    for i in range(60):
        anchor = int((0, 255, rng.integers(1, 255))[i % 3])
        rows = []
        for k in range(3):
            w = rng.random(256) ** 8 + 1e-4
            w[anchor] += (3.0, 1.0, 0.2)[k]
            rows.append(R2.normalise_prior((w * 1e6).astype(np.int64)))
        n = 1 + i % 10
        r = np.clip(anchor + rng.integers(-2, 3, n), 0, 255)
        off = rng.choice(np.array([-0.5, -0.499, -0.25, 0.0, 0.25, 0.499, 0.5]), n)
        f = np.clip((r + off) / 255.0, 0.0, 1.0).astype(np.float32)
        z = np.rint(f * np.float32(255.0)).astype(np.int64)  # a code consistent with f
        cand, D = Q.candidates(z, f)
        yield f"random {i}", cand, D, Q.COST16[np.asarray(rows, np.int64)], anchor


def test_trellis_is_optimal_and_breaks_ties_by_rule(cases, priors):
    chains = list(_fixture_chains(cases, priors[1])) + list(_random_chains())
    moved = ties = 0
    for name, cand, D, cost_rows, anchor in chains:
        for lam in LAMS:
            lam_fix = Q.lam_fix_of(lam)
            choice, total = Q.trellis_chain(cand, D, cost_rows, anchor, lam_fix)
            want, least = _exhaustive(cand, D, cost_rows, anchor, lam_fix)
            assert total == least == Q.chain_cost(choice, cand, D, cost_rows, anchor, lam_fix), (name, lam)
            assert choice == want, (name, lam)
            moved += any(choice)
    # the tie rule decides something: with flat rows every exact .5 tie costs the same either way
    flat = np.full((3, 256), Q.COST16[16])
    r = np.arange(1, 11)
    f = ((r + 0.5) / 255.0).astype(np.float32)
    cand, D = Q.candidates(r, f)
    exact = D[:, 0] == D[:, 1]
    ties = int(exact.sum())
    choice, _ = Q.trellis_chain(cand, D, flat, 5, Q.lam_fix_of(1.0))
    assert choice == _exhaustive(cand, D, flat, 5, Q.lam_fix_of(1.0))[0]
    assert all(b == 0 for b, t in zip(choice, exact) if t)
    print(f"{len(chains)} chains x {len(LAMS)} lambdas, {moved} with a code moved, {ties} exact ties among 10")
    assert moved > 0 and ties > 0


@pytest.mark.parametrize("seg_pixels", (5, 32))
def test_vectorised_pass_is_the_scalar_chain(cases, priors, seg_pixels):
    anchors, freqs = priors[1]
    cost = Q.COST16[np.asarray(freqs, np.int64)]
    for name, lam in (("odd37x53", 1.0), ("imagenet4_trained", 0.1)):
        z, f = cases[name]["latent"][0], cases[name]["prequant"][0]
        lam_fix = Q.lam_fix_of(lam)
        got = Q.rdoq_context(z, f, priors[1], lam_fix, seg_pixels).reshape(-1, Q.CH)
        cand, D = Q.candidates(z.reshape(-1, Q.CH), f.reshape(-1, Q.CH))
        for s0 in range(0, len(cand), seg_pixels):
            for c in range(Q.CH):
                choice, _ = Q.trellis_chain(cand[s0:s0 + seg_pixels, c], D[s0:s0 + seg_pixels, c], cost[c], int(anchors[c]), lam_fix)
                want = [int(cand[s0 + p, c, b]) for p, b in enumerate(choice)]
                assert got[s0:s0 + seg_pixels, c].tolist() == want, (name, s0, c)


@pytest.mark.parametrize("case", CASES)
def test_priced_cost_never_rises_and_codes_move_one_step_at_most(cases, priors, case):
    static, cprior = priors
    for z, f in zip(cases[case]["latent"], cases[case]["prequant"]):
        for lam in LAMS:
            lam_fix = Q.lam_fix_of(lam)
            z2 = Q.rdoq_static(z, f, static, lam_fix)
            assert np.abs(z2.astype(int) - z.astype(int)).max() <= 1
            cand, D = Q.candidates(z, f)
            cost = Q.COST16[np.asarray(static, np.int64)][np.arange(Q.CH), :]
            j_in = D[..., 0] + lam_fix * cost[np.arange(Q.CH), z.astype(np.int64)]
            moved = z2 != z
            j_out = np.where(moved, D[..., 1], D[..., 0]) + lam_fix * cost[np.arange(Q.CH), z2.astype(np.int64)]
            assert (j_out <= j_in).all() and (j_out[moved] < j_in[moved]).all()  # a tie stays at r
            assert Q.priced_cost_static(z2, f, static, lam_fix) == int(j_out.sum())
            for sp in (5, 32):
                z3 = Q.rdoq_context(z, f, cprior, lam_fix, sp)
                assert np.abs(z3.astype(int) - z.astype(int)).max() <= 1
                before, after = _chain_costs(z, f, cprior, lam_fix, sp), _chain_costs(z3, f, cprior, lam_fix, sp)
                assert (after <= before).all()
                assert Q.priced_cost_context(z3, f, cprior, lam_fix, sp) == int(after.sum())


def test_it_pays_in_real_bytes(cases, priors):
    """kodim21_256_trained under the priors of the four imagenet4_trained latents, seg_pixels 32."""
    static, cprior = priors
    z, f = cases["kodim21_256_trained"]["latent"][0], cases["kodim21_256_trained"]["prequant"][0]
    lam_fix = Q.lam_fix_of(0.05)
    z3, z2 = Q.rdoq_context(z, f, cprior, lam_fix, 32), Q.rdoq_static(z, f, static, lam_fix)
    v3 = [len(R3.write_file(a, cprior, 32)) for a in (z, z3)]
    v2 = [len(R2.write_file(a, static, 32)) for a in (z, z2)]
    print(f"version 3: {v3[0]} -> {v3[1]} B, {100 * np.mean(z3 != z):.2f} % of codes changed; version 2: {v2[0]} -> {v2[1]} B, "
          f"{100 * np.mean(z2 != z):.2f} % changed")
    assert v3 == [4850, 4704]  # the prototype's figures
    assert v3[1] < v3[0]
    assert v2[1] <= v2[0]


@pytest.mark.parametrize("case", CASES)
def test_files_of_the_chosen_codes_round_trip(cases, priors, case):
    static, cprior = priors
    z, f = cases[case]["latent"][0], cases[case]["prequant"][0]
    lam_fix = Q.lam_fix_of(0.1)
    z3, z2 = Q.rdoq_context(z, f, cprior, lam_fix, 32), Q.rdoq_static(z, f, static, lam_fix)
    assert (z3 != z).any() and (z2 != z).any()
    np.testing.assert_array_equal(R3.read_file(R3.write_file(z3, cprior, 32), cprior), z3)
    np.testing.assert_array_equal(R2.read_file(R2.write_file(z2, static, 32), static), z2)


def test_the_reference_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        Q.lam_fix_of(-0.01)
    with pytest.raises(ValueError):
        Q.lam_fix_of(16.01)
    assert Q.lam_fix_of(16.0) == 16 << 16
    z = np.zeros((1, 1, 96), np.uint8)
    with pytest.raises(ValueError):
        Q.rdoq_context(z, z.astype(np.float32), R3.uniform_context_prior(), 0, 65)


def test_argument_checks_come_before_any_gpu_call():
    """Shape, then the empty batch, then NULL: none of these reaches the device (no ctx exists here)."""
    L = _lib.lib()
    assert "nic_rdoq" in _lib.header_symbols()

    def call(n=1, h8=2, w8=2, seg_pixels=32, lam_fix=0, contexts=3, ctx=None, z=None, f=None, out=None):
        return L.nic_rdoq(ctx, z, f, n, h8, w8, seg_pixels, lam_fix, contexts, out, None)

    assert call(n=-1) == _lib.NIC_ESHAPE
    assert call(h8=0) == _lib.NIC_ESHAPE
    for sp in (0, 65, -1, 4096):
        assert call(seg_pixels=sp) == _lib.NIC_ESHAPE
        assert "1..64" in _lib.last_error()
        assert call(seg_pixels=sp, contexts=1) == _lib.NIC_ESHAPE
    assert call(lam_fix=(16 << 16) + 1) == _lib.NIC_EINVAL
    assert call(contexts=2) == _lib.NIC_EINVAL
    assert call(n=0) == _lib.NIC_OK  # an empty batch is OK, before the NULL checks
    assert call(n=0, seg_pixels=65) == _lib.NIC_ESHAPE
    for sp in (1, 64):
        assert call(seg_pixels=sp, lam_fix=16 << 16) == _lib.NIC_EINVAL
        assert "NULL ctx" in _lib.last_error()


class _NoGpu:
    """Stands in for an Encoder: use_model must refuse before it touches the model."""

    class codec:
        prior = None
        context_prior = None
        RDOQ_LAM_MAX = 16.0

    def load(self, path):
        raise AssertionError("use_model went on to load the checkpoint")


def test_the_driver_refuses_rdoq_without_its_needs(tmp_path):
    src = str(tmp_path)
    with pytest.raises(ValueError, match='container="nic"'):
        B.use_model(_NoGpu(), src, "ckpt", src + "_out", in_cshape=3, rdoq=0.05)
    with pytest.raises(ValueError, match='container="nic"'):
        B.use_model(_NoGpu(), src, "ckpt", src + "_out", in_cshape=96, container="nic", rdoq=0.05)
    with pytest.raises(ValueError, match="needs a prior"):
        B.use_model(_NoGpu(), src, "ckpt", src + "_out", in_cshape=3, container="nic", rdoq=0.05)

    class WithPrior(_NoGpu):
        class codec(_NoGpu.codec):
            prior = object()

    for lam in (-0.01, 16.5, float("nan")):
        with pytest.raises(ValueError, match="not in"):
            B.use_model(WithPrior(), src, "ckpt", src + "_out", in_cshape=3, container="nic", rdoq=lam)
