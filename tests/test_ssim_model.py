"""The fp32 arithmetic of the MS-SSIM kernels (tests/ssim_f32_model.py, a CPU restatement of
csrc/nic_quality.hip) against the float64 oracle, on the cases of tests/ssim_cases.py.

Two things are held here, without a GPU:
  * the new flat cases discriminate: with the fixed shift of 0.5 that the kernel used to
    subtract, the model misses the 2e-6 contract on them;
  * with the shift the kernel subtracts now (the mean of each tile's window) the model keeps
    the contract on every new case, and the tighter relative bound on the 1-pixel cross.
The device itself is checked in test_gpu_quality.py, against the oracle and not this model.

Model max |d| vs oracle, terms / result:
  case                      fixed 0.5            window mean
  flat_254_noise1           5.7e-05 / 3.3e-06    1.9e-07 / 2.9e-08
  bright_250_255_noise2     4.3e-05 / 3.1e-06    1.2e-07 / 1.8e-09
  dark_0_5_noise2           2.6e-05 / 5.9e-07    8.4e-08 / 5.5e-09
  const_255_vs_254          3.3e-05 / 3.3e-05    6.0e-08 / 4.4e-08
  const_0_vs_1              6.0e-08 / 8.0e-08    6.0e-08 / 8.0e-08
  const_255_identical       6.0e-08 / 6.0e-08    6.0e-08 / 6.0e-08
  ramp_200_255_noise1       1.2e-05 / 2.0e-07    1.0e-07 / 1.8e-08
  halves_0_255_noise1       1.2e-05 / 6.0e-06    1.1e-05 / 1.1e-06
  batch_black_white_noise   4.0e-05 / 2.0e-05    1.4e-07 / 5.4e-08
const_0_vs_1 does not strain the fixed form: 0 - 0.5 is exact and 1/255 - 0.5 is a constant, and
the FMA chains over a constant image round the same way in both moments.  An earlier estimate of
6.6e-5 for this case, from a model without FMA emulation, could not be reproduced: this model and
the device both give 6e-8 under the fixed 0.5.  Neither it nor the identical pair is asserted to
fail under 0.5.  halves_0_255_noise1 is in the list below through its result (6.0e-6 under 0.5);
its terms move little (1.2e-5 to 1.1e-5) and keep a bound of their own, C.OWN_TERM_ATOL.
"""
import numpy as np
import pytest

from tests import ssim_cases as C
from tests import ssim_f32_model as M

ADOPTED = "window_mean"  # the form of ssim_tile_kernel; "fixed" here fails the tests below

# flat cases on which the fixed 0.5 must miss the contract (see the table above)
DISCRIMINATING = ["flat_254_noise1", "bright_250_255_noise2", "dark_0_5_noise2", "const_255_vs_254",
                  "ramp_200_255_noise1", "halves_0_255_noise1", "batch_black_white_noise"]


def _err(name, shift):
    a, b = C.all_pairs()[name]
    ref, ref_terms = C.oracle_of(name)
    got, terms = M.ms_ssim(a, b, shift)
    return float(np.abs(terms - ref_terms).max()), float(np.abs(got - ref).max()), got, terms


@pytest.mark.parametrize("case", DISCRIMINATING)
def test_fixed_half_shift_misses_contract(case):
    dt, dr, _, _ = _err(case, "fixed")
    print(f"{case}: fixed 0.5: terms max|d| {dt:.2e} ms_ssim max|d| {dr:.2e}")
    assert max(dt, dr) > C.ATOL


@pytest.mark.parametrize("case", sorted(C.all_pairs()))
def test_adopted_shift_keeps_contract(case):
    dt, dr, got, terms = _err(case, ADOPTED)
    print(f"{case}: {ADOPTED}: terms max|d| {dt:.2e} ms_ssim max|d| {dr:.2e}")
    assert dt <= C.OWN_TERM_ATOL.get(case, C.ATOL)  # one case's terms have their own bound
    assert dr <= C.ATOL
    if case == "const_255_identical":
        np.testing.assert_allclose(got, 1.0, rtol=0, atol=1e-6)
    if case == "relu_inverted":
        assert (C.oracle_of(case)[1][:, :, :4, 1] < 0).all() and (got == 0.0).all()
    if case == "cross_row37_col37":
        assert C.cross_excess(terms, C.oracle_of(case)[1]) <= 0.0


def test_shift_is_per_plane():
    """A plane's terms do not depend on what else is in the batch."""
    a, b = C.all_pairs()["batch_black_white_noise"]
    _, whole = M.ms_ssim(a, b, ADOPTED)
    for i in range(a.shape[0]):
        _, one = M.ms_ssim(a[i:i + 1], b[i:i + 1], ADOPTED)
        np.testing.assert_array_equal(one[0], whole[i])


def test_model_rejects_unknown_shift():
    a, b = C.all_pairs()["const_255_identical"]
    with pytest.raises(ValueError):
        M.ms_ssim(a, b, "per_image")
