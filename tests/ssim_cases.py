"""Seeded MS-SSIM image pairs where the device's fp32 arithmetic is under most strain: flat,
near-black and near-white content (local variance far below c2 = 9e-4, so the variance term
is what is left of a cancellation), tile-edge geometry, a negative mean cs, and a difference
confined to a 1-pixel cross.  Shared by test_ssim_model.py (CPU model of the kernel) and
test_gpu_quality.py (the device), both against the float64 oracle."""
import functools

import numpy as np

H, W = 176, 192  # 6 x 6 output tiles at scale 0, an 11 x 12 image at scale 4

ATOL = 2e-6  # the contract of test_gpu_quality.py, per image and per scale term
# The one case whose per-scale terms keep their own bound (twice the figure measured on the
# MI355X, see the table in test_gpu_quality.py): each window across the seam holds flat black and
# flat white, both 0.5 from any one shift, so its flat pixels keep the error of the fixed 0.5.
# For the terms only: the result of this case (1.1e-6) is held to ATOL like every other.  The old
# fixed-0.5 kernel (1.2e-5 on these terms) would pass this bound too; its result (6.0e-6) would not.
OWN_TERM_ATOL = {"halves_0_255_noise1": 2.2e-5}  # measured 1.11e-5, CPU model 1.11e-5


@functools.lru_cache(maxsize=None)
def all_pairs():
    """Every new case by name; built once and shared, so treat the arrays as read-only."""
    out = dict(flat_pairs())
    out.update(geometry_pairs())
    out["relu_inverted"] = relu_pair()
    out["cross_row37_col37"] = cross_pair()
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """(ms_ssim (N,), terms (N,3,5,2)) of the float64 oracle for a case of all_pairs()."""
    from oracle import nic_oracle as O
    a, b = all_pairs()[name]
    return O.ms_ssim(a, b), O.ms_ssim_terms(a, b)


def _noisy(a, amp, rng):
    return np.clip(a.astype(int) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)


def flat_pairs():
    """Flat and extreme content.  Every image is (N, 176, 192, 3) u8."""
    rng = np.random.default_rng(2024)
    shape = (1, H, W, 3)
    const = lambda v: np.full(shape, v, np.uint8)  # noqa: E731
    bright = rng.integers(250, 256, shape, dtype=np.uint8)
    dark = rng.integers(0, 6, shape, dtype=np.uint8)
    ramp = np.broadcast_to(np.linspace(200, 255, W).round().astype(np.uint8)[None, None, :, None], shape).copy()
    halves = np.zeros(shape, np.uint8)
    halves[:, :, W // 2:] = 255  # the seam at x = 96: windows of every scale hold both extremes
    noise = rng.integers(0, 256, shape, dtype=np.uint8)
    mixed = np.concatenate([const(0), const(255), noise])
    return {
        "flat_254_noise1": (const(254), _noisy(const(254), 1, rng)),
        "bright_250_255_noise2": (bright, _noisy(bright, 2, rng)),
        "dark_0_5_noise2": (dark, _noisy(dark, 2, rng)),
        "const_255_vs_254": (const(255), const(254)),
        "const_0_vs_1": (const(0), const(1)),
        "const_255_identical": (const(255), const(255)),
        "ramp_200_255_noise1": (ramp, _noisy(ramp, 1, rng)),
        "halves_0_255_noise1": (halves, _noisy(halves, 1, rng)),
        "batch_black_white_noise": (mixed, _noisy(mixed, 1, rng)),
    }


def geometry_pairs():
    """168x172: scale 2 is 42x43, so 32x33 outputs, exactly one tile row and a second tile column
    of one pixel; scale 4 is 11x11, a single output.  161x700: one long row of tiles."""
    rng = np.random.default_rng(2025)
    a = rng.integers(0, 256, (1, 168, 172, 3), dtype=np.uint8)
    b = _noisy(a, 12, rng)
    wide = rng.integers(0, 256, (1, 161, 700, 3), dtype=np.uint8)
    return {
        "tile_edge_168x172": (a, b),
        "tile_edge_172x168": (a.transpose(0, 2, 1, 3).copy(), b.transpose(0, 2, 1, 3).copy()),
        "wide_161x700": (wide, _noisy(wide, 12, rng)),
    }


def relu_pair():
    """b = 255 - a on noise: the mean cs of scales 0..3 is negative in every channel (at scale 4
    the pooled noise is nearly grey and cs turns positive), so the relu makes the result exactly 0."""
    a = np.random.default_rng(2026).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    return a, 255 - a


def cross_pair():
    """b = a except along row y = 37 and column x = 37: at scale 0 the outputs that see the
    difference are 27..37 in each direction, across the tile seam at 32."""
    rng = np.random.default_rng(2027)
    a = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    b = a.copy()
    b[:, 37, :, :] = rng.integers(0, 256, b[:, 37, :, :].shape, dtype=np.uint8)
    b[:, :, 37, :] = rng.integers(0, 256, b[:, :, 37, :].shape, dtype=np.uint8)
    return a, b


# |(1 - got) - (1 - ref)| <= CROSS_RTOL * (1 - ref) + CROSS_ATOL per term of cross_pair():
# 1e-4 is 50 times the fp32-class relative error (2e-6 on terms of order 1) of the other cases;
# 2.4e-7 is two fp32 ulps of a returned term near 1
CROSS_RTOL, CROSS_ATOL = 1e-4, 2.4e-7


def cross_excess(got_terms, ref_terms):
    """max over terms of |(1 - got) - (1 - ref)| - (CROSS_RTOL * (1 - ref) + CROSS_ATOL); <= 0 passes."""
    d = np.abs((1.0 - got_terms.astype(np.float64)) - (1.0 - ref_terms))
    return float((d - (CROSS_RTOL * np.abs(1.0 - ref_terms) + CROSS_ATOL)).max())
