"""The range-guard cases of tests/range_sites.py do what they claim, in the float64 oracle:
the target site is far over the f16 limit, every other split site of the pass far under it,
position cases are confined to their pixel's receptive field, exact-compensation cases leave
the outputs bit-identical.  The low-side cases (range_sites.low_cases) are held to the same
standard, and tests/split_f16_model.py's prediction of what the split loses on them is pinned
down.  No GPU: tests/test_gpu_range_sites.py runs the same cases on it."""
from functools import lru_cache

import numpy as np
import pytest

from oracle import nic_oracle as O
from tests import range_sites as R
from tests import split_f16_model as M

CASES = R.all_cases()


def _plane_max(acts, planes, site):
    return max(float(np.abs(acts[p][site]).max()) for p in planes)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_conditions(case):
    acts = case.activations()
    target_planes = R.PLANES[case.model]
    # the Cr planes (the last of the batch) carry the CbCr cases; Y its own plane
    top = _plane_max(acts, target_planes[-1:], case.site)
    print(f"\n{case.name}: target {case.site} max {top:.4g} = {top / R.LIMIT:.2f} x limit")
    assert np.isfinite(top)
    if case.below:
        assert R.LIMIT / 2 <= top < R.LIMIT
    else:
        assert top >= 2 * R.LIMIT  # past 65520: a missed guard yields inf, not a harmless 65504
    if case.cr_only:
        assert _plane_max(acts, (1,), case.site) <= R.LIMIT / 2
    # every other split site, and the target site under the other model, stays far below
    for p in range(3):
        for site in R.SPLIT_SITES[case.direction]:
            if site == case.site and p in target_planes:
                continue
            m = float(np.abs(acts[p][site]).max())
            assert m <= R.LIMIT / 2, (p, site, m)
    if case.kind == "position":
        n = case.x.shape[0]
        over = np.concatenate([np.abs(acts[p][case.site]).max(axis=3) >= R.LIMIT for p in target_planes])
        h, w = over.shape[1:]
        assert h * w > 1
        yy, xx = np.mgrid[0:h, 0:w]
        near = (np.abs(yy - case.centre[0]) <= case.radius) & (np.abs(xx - case.centre[1]) <= case.radius)
        plane = (case.plane - target_planes[0]) * n + case.image
        allowed = np.zeros_like(over)
        allowed[plane] = near
        assert not np.any(over & ~allowed)
        a = np.abs(acts[case.plane][case.site][case.image]).max(axis=2)
        for y, x in case.cover:
            assert a[y, x] >= 2 * R.LIMIT, (y, x, a[y, x])
        # no value sits at the limit itself (the device agrees with the oracle to ~1e-5 relative)
        assert not np.any((a < 1.001 * R.LIMIT) & (a > 0.999 * R.LIMIT))
    if case.kind == "exact":
        np.testing.assert_array_equal(case.outputs(), case.outputs(case.base))
    if case.share:
        rf = case.outputs()
        assert np.mean((rf > 0) & (rf < 1)) >= 0.80


def test_every_site_and_form_is_covered():
    """Every row of the split-site table: conv1, conv2, dconv1, dconv7 once, the four k3 sites in
    the fused pair, the strip pair and the two-launch form; each kernel under both models."""
    sites = {(c.site, c.shape) for c in R.site_cases()}
    for site, shapes in (("conv3", (R.E_PAIR, R.E_WS, R.E_STRIP)), ("conv4", (R.E_PAIR, R.E_WS, R.E_STRIP)),
                         ("dconv5", (R.D_PAIR, R.D_WS, R.D_STRIP)), ("dconv6", (R.D_PAIR, R.D_WS, R.D_STRIP))):
        for shape in shapes:
            assert (site, shape) in sites
    assert {"conv1", "conv2", "dconv1", "dconv7"} <= {c.site for c in R.site_cases()}
    kernel = {"conv1": "conv12", "conv2": "conv12", "dconv1": "dconv1_all", "dconv7": "ws-proj"}
    models = {}
    for c in R.site_cases() + R.position_cases():
        k = kernel.get(c.site) or ("ws" if not c.fused else "strip" if c.shape in (R.E_STRIP, R.D_STRIP) else "pair")
        models.setdefault(k, set()).add(c.model)
    assert models == {k: {"Y", "CbCr"} for k in ("conv12", "pair", "strip", "ws", "ws-proj", "dconv1_all")}
    assert {c.direction for c in R.below_cases()} == {"enc", "dec"}


# ---- the low side ----------------------------------------------------------------------------
LOW = R.low_cases()
CONTRACT = 2e-5  # PREQUANT_ATOL, DECODE_F32_ATOL (tests/test_gpu_parity.py)


@lru_cache(maxsize=None)
def _base(direction, shape):
    """The unscaled spread network on the shape's seeded input: (activations, outputs), once."""
    c = R.Case("base", direction, "", "Y", shape, "exact", R.seeded_input(direction, shape), R.spread_weights())
    return c.activations(), c.outputs()


def test_low_cases_cover_what_they_claim():
    """conv1, conv3, dconv5, dconv7 alone and the whole trunk, each under both models, in the
    fused and the two-launch form, at every level; the trunk's targets are the residual sites."""
    got = {(c.direction, c.targets, c.model, c.shape, c.fused, c.low) for c in LOW}
    assert len(got) == len(LOW) == 2 * 3 * 2 * 2 * len(R.LOW_LEVELS)
    for d in ("enc", "dec"):
        assert {f for _, f in R.LOW_SHAPES[d]} == {True, False}
        for shape, fused in R.LOW_SHAPES[d]:
            for model in ("Y", "CbCr"):
                for k in R.LOW_LEVELS:
                    for t in [(s,) for s in R.LOW_SINGLE[d]] + [R.TRUNK[d][:3]]:
                        assert (d, t, model, shape, fused, k) in got
    assert R.LOW_LEVELS == (4, 8, 12, 17, 24)
    assert set(R.TRUNK["enc"][:3]) >= {"conv2", "conv4"} and set(R.TRUNK["dec"][:3]) >= {"dconv1", "dconv6"}


@pytest.mark.parametrize("case", LOW, ids=[c.name for c in LOW])
def test_low_case_conditions(case):
    base_acts, base_out = _base(case.direction, case.shape)
    acts = case.activations()
    np.testing.assert_array_equal(case.outputs(), base_out)  # bit for bit, every level
    np.testing.assert_array_equal(case.outputs(case.base), base_out)
    down = np.float32(2.0 ** -case.low)
    last = "conv8" if case.direction == "enc" else "dconv8"
    for p in range(3):
        for site in R.SPLIT_SITES[case.direction] + (last,):
            a, b = acts[p][site], base_acts[p][site]
            if site in case.targets and p in R.PLANES[case.model]:
                assert float(np.abs(a).max()) == float(np.abs(b).max()) * float(down)
                np.testing.assert_array_equal(a, b * down)
            else:
                np.testing.assert_array_equal(a, b)
            assert float(np.abs(a).max()) < R.LIMIT / 2  # the high-side guard stays out of it
    if case.direction == "dec":  # the unscaled network on DECODE_FORMS' own inputs
        assert case.share and np.mean((base_out > 0) & (base_out < 1)) >= 0.80


def _low_family(case):
    return case.name.rsplit("-k", 1)[0]


FAMILIES = sorted({_low_family(c) for c in LOW})


@lru_cache(maxsize=None)
def _predicted(family, k):
    """The model's max |delta| at the output for one family at level k (k = 0: nothing scaled)."""
    case = next(c for c in R.low_cases((k,)) if _low_family(c) == family)
    return M.split_error(case, case.targets)


@pytest.mark.parametrize("family", FAMILIES)
def test_split_model_on_the_low_cases(family):
    """What the activation split alone costs, by tests/split_f16_model.py: nothing to speak of on
    the unscaled network (<= 2e-6; the device's whole error is <= 4.4e-6), never
    less as the targets run lower, and at 2^-17 -- the magnitude the high-side cases use upwards --
    every single-site case is past the 2e-5 contract (by two orders of magnitude: 2.4e-3 .. 7.1e-3;
    the trunk 5.1e-3 .. 1.2e-2).  The split pass therefore cannot hold the contract on these
    networks by itself, and nothing on the high side of the guard notices them."""
    errs = [_predicted(family, k) for k in (0,) + R.LOW_LEVELS]
    print(f"\n{family}: " + "  ".join(f"k={k}: {e:.1e}" for k, e in zip((0,) + R.LOW_LEVELS, errs)))
    assert errs[0] <= 2e-6
    assert all(b >= a for a, b in zip(errs, errs[1:]))
    if "trunk" not in family:
        assert errs[1 + R.LOW_LEVELS.index(17)] > CONTRACT


def _fixture_site_minimum(golden, manifest, weights_by_init):
    """The smallest per-site, per-model oracle maximum over every golden and trained fixture."""
    least = (np.inf, None)
    for name, entry in manifest["cases"].items():
        if "init" not in entry or entry["init"] not in weights_by_init:
            continue
        g, w = golden(name), weights_by_init[entry["init"]]
        if "x" not in g or "latent" not in g or g["x"].ndim != 4 or g["x"].shape[1] * g["x"].shape[2] > 1 << 16:
            continue
        for d, acts in (("enc", O.encoder_activations(w, g["x"])), ("dec", O.decoder_activations(w, g["latent"]))):
            for model, planes in R.PLANES.items():
                for site in R.SPLIT_SITES[d]:
                    m = max(float(np.abs(acts[p][site]).max()) for p in planes)
                    least = min(least, (m, f"{name} {model} {site}"))
    return least


def test_a_site_maximum_cannot_separate_the_low_cases_from_the_fixtures(golden, manifest, weights_by_init):
    """Why the low side gets no max-based guard.  A guard "re-run in fp32 when some site's maximum
    is below T" needs T above the site maximum of every low case whose predicted error is past a
    quarter of the contract (5e-6; the rest is the device's own 4.4e-6), and 2^4 of room below the
    smallest site maximum of any shipped fixture.  The model asks for T >= 0.034 (the decoder's
    CbCr trunk at k = 6: 5.3e-6 with dconv5 at 2.2 x 2^-6); the fixtures go down to 0.030 (the
    trained 0.01 encoder's Y conv3, 0.0305; the glorot decoder's dconv7, 0.032).  There is no room
    at all, let alone 2^4: such a guard would trip on shipped fixtures, which hold the contract
    because their next layers are not scaled up to match.  What separates the two is the product
    of a site's scale and the next kernel's, which a maximum of activations does not see."""
    need = 0.0
    for family in FAMILIES:
        for k in range(4, 9):
            if _predicted(family, k) <= CONTRACT / 4:
                continue
            case = next(c for c in R.low_cases((k,)) if _low_family(c) == family)
            need = max(need, min(M.site_maxima(case)[t] for t in case.targets))
    least, where = _fixture_site_minimum(golden, manifest, weights_by_init)
    print(f"\nthreshold needed {need:.4f}; smallest fixture site maximum {least:.4f} ({where})")
    assert 2.0 ** -6 < need < 2.0 ** -4
    assert least < 16 * need  # no room: were this ever false, a max-based guard would be worth another look


def test_lift_leaves_ordinary_weights_alone(weights_by_init):
    """weights.lift_low_sites (what Codec.set_weights uploads) returns every shipped weight set, and
    every high-side case's weights, as they are -- the same arrays: their sites' estimates are at or
    above LIFT_FLOOR, so the high-side cases still trip and the shipped codecs compute the same bits."""
    from neural_network_image_compression_amd import weights as W
    for name, w in weights_by_init.items():
        lifted = W.lift_low_sites(w)
        assert all(lifted[k] is w[k] for k in w), name
        for model in W.MODEL_NAMES:
            assert min(W.site_estimates(w, model)[:-1]) >= W.LIFT_FLOOR, (name, model)
    for case in CASES:
        lifted = W.lift_low_sites(case.weights)
        assert all(lifted[k] is case.weights[k] for k in case.weights), case.name
    part = {k: v for k, v in weights_by_init["spread"].items() if not k.endswith("conv3/bias")}
    assert all(W.lift_low_sites(part)[k] is part[k] for k in part)  # incomplete models: untouched


@pytest.mark.parametrize("case", LOW, ids=[c.name for c in LOW])
def test_lift_restores_the_low_cases(case):
    """The lifted weights are the same network (the oracle's outputs bit for bit, at every level),
    every site's estimate is back at or above LIFT_FLOOR, whatever else was scaled stays put, and
    the split of all four sites together then costs at most a quarter of the contract (measured:
    at most 1.5e-6, against up to 0.80 before the lift)."""
    import dataclasses

    from neural_network_image_compression_amd import weights as W
    _, base_out = _base(case.direction, case.shape)
    lifted = dataclasses.replace(case, weights=W.lift_low_sites(case.weights))
    np.testing.assert_array_equal(lifted.outputs(), base_out)
    model = case.prefix()[:-1]
    e = W.site_lifts(case.weights, model)
    names = [s.name for s in W.layer_table(model)]
    for name, ei in zip(names, e):
        assert case.low - 6 <= ei <= case.low if name in case.targets else ei == 0, (names, e)
    src, dst = (1, 3) if case.direction == "enc" else (0, 2)
    assert e[src] == e[dst] and e[-1] == 0
    est = W.site_estimates(lifted.weights, model)
    assert all(W.LIFT_FLOOR <= m < W.LIFT_CEILING for m in est[:-1])
    other = [k for k in case.weights if not k.startswith(case.prefix())]
    assert all(lifted.weights[k] is case.weights[k] for k in other)
    err = M.split_error(lifted, R.SPLIT_SITES[case.direction])
    assert err <= CONTRACT / 4, err


def test_split_model_primitives():
    """split() is split4: RNE to f16, the exact remainder to f16 with subnormals kept; hi + lo is
    x to 2^-22 relative while lo is normal, and to the fixed 2^-25 once lo is subnormal."""
    x = np.float32([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 3.0 * 2.0 ** -26, 2.0 ** -25, -2.0 ** -26])
    hi, lo = M.split(x)
    assert hi.dtype == lo.dtype == np.float16
    np.testing.assert_array_equal(hi[:3], np.float16([1.0, 1.0, 1.0]))  # ties to even
    np.testing.assert_array_equal(lo[:3].astype(np.float32), np.float32([0, 2.0 ** -11, 2.0 ** -12]))
    np.testing.assert_array_equal(hi[3:6].astype(np.float32), np.float32([2.0 ** -24, 0.0, -0.0]))  # 2^-25: tie to 0
    assert M.merged(x[3:6]).tolist() == [2.0 ** -24, 0.0, 0.0]  # lo cannot bring back what hi lost
    rng = np.random.default_rng(5)
    v = rng.uniform(-4, 4, 4096).astype(np.float32)
    assert np.abs(M.merged(v) - v).max() <= 4 * 2.0 ** -22
    small = v * np.float32(2.0 ** -12)  # |hi| < 2^-10: lo < 2^-21 ... subnormal spacing 2^-24
    err = np.abs(M.merged(small) - small).max()
    assert 2.0 ** -27 < err <= 2.0 ** -25
    tiny = v * np.float32(2.0 ** -26)
    assert np.all(M.split(tiny)[0].astype(np.float32) ** 2 <= (2.0 ** -24) ** 2)  # hi flushed to 0 or one step
