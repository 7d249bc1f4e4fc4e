"""The f16 range guard tripped at every split-f16 site of the f16x3 product path, one site at a
time (cases: tests/range_sites.py, validated on the CPU by tests/test_range_sites.py).

The guard is a chain in which a later site does not back up an earlier one: range_track's
max ignores NaN, and an activation that overflows unseen reaches the next layer as inf - inf.
So each case puts exactly one site over the limit (>= 2 x 65504 in the float64 oracle, every
other split site <= 65504 / 2) and asserts, with the default FALLBACK policy, that
range_trips() rises by exactly 1, that the outputs meet the project's contract against the live
float64 oracle with the case's weights (encoder: PREQUANT_ATOL, check_codes, the codes the exact
quantisation of the floats; decoder: check_recon_f32, and the unclipped share >= SHARE_SPREAD
where the case keeps DECODE_FORMS' input), and that they are bit-identical to a
Codec(precision="fp32") with the same weights (the re-run is those kernels: a partial re-run
or a stale plane shows here even where the output is clipped); then, with the ERROR policy,
that the call raises NIC_ERANGE and range_trips() rises by 1 again.  The form of the k3 pair is
asserted through the launch count of conv3 / dconv5.  Below-limit cases (the target's max in
[65504 / 2, 65504)) must not trip and must meet the same contract from the split pass itself.

Measured on the MI355X, max |delta| against the float64 oracle (bound 2e-5 throughout; the
tripped cases are the exact-fp32 re-run's outputs):
  site cases:      conv1-CbCr-2x24x130 8.3e-7   conv2-Y-2x24x469 1.3e-6     conv3-Y-2x24x130 4.8e-7
                   conv3-CbCr-1x24x257 7.2e-7   conv3-CbCr-2x24x469 7.8e-7  conv4-CbCr-2x24x130 8.3e-7
                   conv4-Y-1x24x257 4.2e-7      conv4-Y-2x24x469 4.8e-7     dconv1-Y-2x3x9 2.2e-6
                   dconv5-CbCr-2x3x9 1.3e-6     dconv5-Y-1x3x33 1.2e-6      dconv5-Y-2x3x59 1.3e-6
                   dconv6-Y-2x3x9 1.0e-6        dconv6-CbCr-1x3x33 9.8e-7   dconv6-CbCr-2x3x59 1.1e-6
                   dconv7-Y-2x3x9 1.3e-6
  position cases:  conv1-last-pixel 4.8e-7      dconv1-last-pixel 8.9e-8    pair-a-last-pixel 2.1e-7
                   pair-b-last-pixel 2.1e-7     pair-a-range-boundary 3.0e-7  strip-a-last-pixel 2.1e-7
                   strip-b-last-pixel 2.1e-7    strip-a-seam 3.6e-7         strip-b-seam 2.1e-7
                   ws-a-last-pixel 2.1e-7       ws-b-last-pixel 2.1e-7      dconv7-last-pixel 2.7e-7
  below the limit: conv3-Y-2x24x130-below 2.7e-7   dconv7-CbCr-2x3x9-below 7.2e-7   (the split pass itself)
No purpose-built network needed a bound of its own: the largest, dconv1-Y-2x3x9, is a ninth of
2e-5.  The decoder site cases' unclipped share is 0.85 .. 0.96 (bounded >= SHARE_SPREAD where the
input is DECODE_FORMS' own); the position cases' outputs are unclipped throughout (one latent
pixel, the rest of the image at the biases' level) and get no share bound.

The low side (range_sites.low_cases: the same sites scaled down by 2^-k, the next kernel up by
2^k, the oracle's outputs those of the unscaled network bit for bit) is held to the same contract
in both precision modes by test_low_side_holds_the_contract; its figures are in its docstring.
"""
import numpy as np
import pytest

from oracle import nic_oracle as O
from tests import range_sites as R
from tests.test_gpu_parity import (DECODE_F32_ATOL, PREQUANT_ATOL, SHARE_SPREAD, _dev, _launches, check_codes,
                                   check_recon, check_recon_f32, report_recon_f32)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_REF = {}


def _oracle(case):
    """The float64 oracle's output with the case's weights, once per case."""
    if case.name not in _REF:
        _REF[case.name] = case.outputs()
        _REF[case.name].setflags(write=False)
    return _REF[case.name]


def _run(c, case, timed_layer=None):
    x = _dev(case.x)
    call = (lambda: c.encode(x, prequant=True)) if case.direction == "enc" else (lambda: c.decode(x, rgb_f32=True))
    if timed_layer is None:
        out, launches = call(), None
    else:
        out, launches = _launches(c, timed_layer, call)
    return tuple(t.cpu().numpy() for t in out), launches


def check_case(case):
    """One case under both policies (also run by tests/range_guard_check.py in a child process
    under the re-run's load-time switches).  Returns max |delta| against the oracle."""
    from neural_network_image_compression_amd import _lib
    from neural_network_image_compression_amd.codec import Codec
    c = Codec(0)
    assert c.precision == "f16x3"
    c.set_weights(case.weights)
    ref = _oracle(case)
    (q, f), launches = _run(c, case, "conv3" if case.direction == "enc" else "dconv5")
    assert launches == (0 if case.fused else 1), "the shape no longer selects the form the case is for"
    trips = c.range_trips()
    assert q.shape == ref.shape[:3] + (q.shape[3],) and f.shape == ref.shape
    worst = float(np.abs(f.astype(np.float64) - ref).max())
    share = float(np.mean((ref > 0) & (ref < 1)))
    print(f"\nrange-site {case.name} ({case.kind}): trips {trips}, max|delta| {worst:.2e}, unclipped {share:.3f}")
    assert trips == (0 if case.below else 1)
    if case.direction == "enc":
        assert worst <= PREQUANT_ATOL
        check_codes(q, O.quantise_u8(ref), ref)
        np.testing.assert_array_equal(O.quantise_u8(f), q)
    else:
        check_recon_f32(f, q, ref, DECODE_F32_ATOL)
        if case.share:
            assert share >= SHARE_SPREAD
    if case.below:
        c.set_range_policy("error")  # the synchronising check: no trip, no error
        (q2, f2), _ = _run(c, case)
        assert c.range_trips() == 0 and np.array_equal(q2, q) and np.array_equal(f2, f)
        return worst
    exact = Codec(0, precision="fp32")
    exact.set_weights(case.weights)
    (qe, fe), _ = _run(exact, case)
    np.testing.assert_array_equal(q, qe)
    np.testing.assert_array_equal(f, fe)
    c.set_range_policy("error")
    with pytest.raises(_lib.NicError) as e:
        _run(c, case)
    assert e.value.code == _lib.NIC_ERANGE
    assert c.range_trips() == 2
    return worst


SITE, POSITION, BELOW = R.site_cases(), R.position_cases(), R.below_cases()


@pytest.mark.parametrize("case", SITE, ids=[c.name for c in SITE])
def test_site_trips_alone(case):
    """Every row of DESIGN.md's split-site table, the k3 sites in all three forms."""
    check_case(case)


@pytest.mark.parametrize("case", POSITION, ids=[c.name for c in POSITION])
def test_site_trips_at_the_plane_edge(case):
    """Over-limit values only around the last row and column of the last plane of the last
    image, at the strip seam, or on rows a block-range boundary recomputes: a range_track behind
    a tile-edge predicate that leaves those out does not trip."""
    check_case(case)


LOW = R.low_cases()


@pytest.fixture(scope="module", params=["f16x3", "fp32"])
def precision(request):
    return request.param


def _low_oracle(case):
    """The low cases' oracle outputs are the unscaled spread network's on the shape's seeded input,
    bit for bit (tests/test_range_sites.py test_low_case_conditions): one oracle run per shape."""
    key = ("low", case.direction, case.shape)
    if key not in _REF:
        _REF[key] = case.outputs(case.base)
        _REF[key].setflags(write=False)
    return _REF[key]


def _low_contract(what, c, q, f, ref, direction):
    """The project's contract against the oracle; the figure is printed before anything asserts."""
    worst = float(np.abs(f.astype(np.float64) - ref).max())
    print(f"\nlow-side {what} {c.precision}: trips {c.range_trips()}, max|delta| {worst:.2e}")
    if direction == "enc":
        assert worst <= PREQUANT_ATOL
        check_codes(q, O.quantise_u8(ref), ref)
        np.testing.assert_array_equal(O.quantise_u8(f), q)
    else:
        report_recon_f32(what, c, f, q, ref, SHARE_SPREAD)
        check_recon(q, O.quantise_u8(ref))
    return worst


@pytest.mark.parametrize("case", LOW, ids=[c.name for c in LOW])
def test_low_side_holds_the_contract(case, precision):
    """A site that runs at 2^-k, the next kernel larger by 2^k (tests/range_sites.py low_cases): the
    same function, the oracle's outputs unchanged, so the same contract -- from the split pass
    itself or from a re-run in fp32, never a wrong answer.  FALLBACK: the outputs meet the contract;
    a pass that tripped is bit-identical to fp32 mode's.  ERROR: NIC_ERANGE, or success and the same
    contract.  k = 4 does not trip, fp32 mode never does.

    Codec.set_weights lifts every small site by an exact power of two first (weights.lift_low_sites:
    the same function, bit for bit in fp32), so the split pass itself holds the contract and nothing
    trips.  Measured on the MI355X, max |delta| against the oracle, range_trips() 0 in every run
    (the full table is in DESIGN.md section 3, "The low side of the f16 range"):
      f16x3, every level: 3.6e-7 .. 5.4e-7 (encoder), 6.6e-7 .. 2.1e-6 (decoder)
      fp32,  every level: 4.8e-7 .. 5.1e-7 (encoder), 1.2e-6 (decoder)
    Without the lift (set_tensor's path: the tensors as given) the f16x3 figures were, worst case
    per level:  k = 4: 6.0e-7 enc, 1.3e-6 dec     k = 8: 1.2e-5 enc, 1.8e-5 dec
         k = 12: 1.8e-4 enc, 3.6e-4 dec    k = 17: 6.6e-3 enc, 1.15e-2 dec    k = 24: 0.53 enc, 0.80 dec
    (best case: k = 12: 7.8e-5, k = 17: 2.4e-3, k = 24: 0.25), no trip, the device following
    tests/split_f16_model.py to two digits (conv3-Y-2x24x130 at k = 17: model 2.6e-3, device
    2.55e-3): all 72 f16x3 cases at k = 12, 17 and 24 failed the 2e-5 contract."""
    from neural_network_image_compression_amd import _lib
    from neural_network_image_compression_amd.codec import Codec
    c = Codec(0, precision=precision)
    c.set_weights(case.weights)
    ref = _low_oracle(case)
    what = case.name
    (q, f), launches = _run(c, case, "conv3" if case.direction == "enc" else "dconv5")
    assert launches == (0 if case.fused and precision == "f16x3" else 1), "the shape no longer selects the form"
    assert q.shape == ref.shape[:3] + (q.shape[3],) and f.shape == ref.shape
    trips = c.range_trips()
    _low_contract(what, c, q, f, ref, case.direction)
    assert trips in (0, 1)
    if precision == "fp32" or case.low == 4:
        assert trips == 0
    if trips:
        exact = Codec(0, precision="fp32")
        exact.set_weights(case.weights)
        (qe, fe), _ = _run(exact, case)
        np.testing.assert_array_equal(q, qe)
        np.testing.assert_array_equal(f, fe)
    c.set_range_policy("error")
    try:
        (q2, f2), _ = _run(c, case)
    except _lib.NicError as e:
        assert e.code == _lib.NIC_ERANGE and precision == "f16x3" and case.low != 4
        assert c.range_trips() == trips + 1
    else:
        _low_contract(what + " (error policy)", c, q2, f2, ref, case.direction)
        assert c.range_trips() == trips


@pytest.mark.parametrize("case", BELOW, ids=[c.name for c in BELOW])
def test_no_false_trip_below_the_limit(case):
    """The target's max in [65504 / 2, 65504): no trip, and the split pass itself meets the
    contract at the top of the f16 range."""
    check_case(case)
