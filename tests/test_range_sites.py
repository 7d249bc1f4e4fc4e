"""The range-guard cases of tests/range_sites.py do what they claim, in the float64 oracle:
the target site is far over the f16 limit, every other split site of the pass far under it,
position cases are confined to their pixel's receptive field, exact-compensation cases leave
the outputs bit-identical.  No GPU: tests/test_gpu_range_sites.py runs the same cases on it."""
import numpy as np
import pytest

from tests import range_sites as R

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
