"""CPU tests of the oracle itself: two independent restatements must agree, TF-SAME
geometry, adjointness of the transposed conv, the golden fixtures, integer stages."""
import numpy as np
import pytest
import torch

from oracle import nic_oracle as O
from tests import torch_ref as T


@pytest.mark.parametrize("n,k,s,expect", [
    (256, 5, 2, (128, 1, 2)), (255, 5, 2, (128, 2, 2)), (64, 3, 1, (64, 1, 1)),
    (33, 5, 2, (17, 2, 2)), (1, 5, 2, (1, 2, 2)), (2, 5, 2, (1, 1, 2)),
])
def test_same_pads(n, k, s, expect):
    assert O.same_pads(n, k, s) == expect


@pytest.mark.parametrize("h,w,k,s,cin,cout", [
    (16, 16, 5, 2, 3, 8), (15, 17, 5, 2, 4, 4), (9, 6, 3, 1, 5, 7), (1, 3, 5, 2, 2, 3)])
def test_conv_same_matches_torch(h, w, k, s, cin, cout):
    rng = np.random.default_rng(h * 100 + w)
    x = rng.standard_normal((2, h, w, cin)).astype(np.float32)
    kern = rng.standard_normal((k, k, cin, cout)).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    a = O.leaky(O.conv2d_same(x, kern, s) + bias)
    b = T.conv(torch.from_numpy(x).permute(0, 3, 1, 2).double(), kern, bias, s).permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(a, b, rtol=0, atol=2e-6 * np.abs(b).max())


@pytest.mark.parametrize("h,w,k,s,cin,cout", [(8, 8, 5, 2, 3, 6), (5, 7, 5, 2, 4, 2), (6, 9, 3, 1, 3, 5)])
def test_conv_transpose_same_matches_torch(h, w, k, s, cin, cout):
    rng = np.random.default_rng(h * 10 + w)
    x = rng.standard_normal((2, h, w, cin)).astype(np.float32)
    kern = rng.standard_normal((k, k, cout, cin)).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    a = O.leaky(O.conv2d_transpose_same(x, kern, s) + bias)
    b = T.tconv(torch.from_numpy(x).permute(0, 3, 1, 2).double(), kern, bias, s).permute(0, 2, 3, 1).numpy()
    assert a.shape == (2, h * s, w * s, cout)
    np.testing.assert_allclose(a, b, rtol=0, atol=2e-6 * np.abs(b).max())


@pytest.mark.parametrize("n,k,s", [(8, 5, 2), (10, 3, 1), (6, 5, 2)])
def test_conv_transpose_is_adjoint_of_same_conv(n, k, s):
    """Conv2DTranspose(SAME) is the input-gradient of Conv2D(SAME) on the n*s input."""
    rng = np.random.default_rng(n)
    big = rng.standard_normal((1, n * s, n * s, 3))
    small = rng.standard_normal((1, n, n, 4))
    kern_hwio = rng.standard_normal((k, k, 3, 4))
    fwd = O.conv2d_same(big.astype(np.float32), kern_hwio.astype(np.float32), s, acc=np.float64)
    # same kernel viewed as Conv2DTranspose (kh, kw, Cout=3, Cin=4)
    adj = O.conv2d_transpose_same(small.astype(np.float32), kern_hwio.astype(np.float32), s, acc=np.float64)
    lhs = float(np.sum(fwd.astype(np.float64) * small.astype(np.float32)))
    rhs = float(np.sum(big.astype(np.float32).astype(np.float64) * adj))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0)


def test_full_encoder_decoder_match_torch(golden, weights_spread):
    g = golden("imagenet4")
    x = g["x"][:2]
    a = O.encode_f32(weights_spread, x)
    b = T.encode_f32(weights_spread, x)
    assert np.abs(a - b).max() <= 2e-6
    z = O.quantise_u8(a)
    y_o, cb_o, cr_o = O.run_model(weights_spread, "decoder",
                                  [O.normalise_u8(z)[..., 32 * i:32 * i + 32] for i in range(3)])
    planes_t = T.decode_planes(weights_spread, z)
    for po, pt in zip((y_o, cb_o, cr_o), planes_t):
        assert np.abs(po - pt.permute(0, 2, 3, 1).numpy()).max() <= 2e-6


@pytest.mark.parametrize("case", ["kodim21_256", "imagenet4", "odd37x53", "kodim21_glorot", "kodim21_256_trained",
                                  "imagenet4_trained", "kodim21_256_trained_c0.02", "imagenet4_trained_c0.02",
                                  "kodim21_256_trained_c0.03", "imagenet4_trained_c0.03"])
def test_oracle_reproduces_golden(case, golden, manifest, weights_by_init):
    g = golden(case)
    w = weights_by_init[manifest["cases"][case]["init"]]
    f = O.encode_f32(w, g["x"])
    assert np.abs(f - g["prequant"]).max() <= 1e-6
    z = O.quantise_u8(f)
    diff = z.astype(int) - g["latent"].astype(int)
    assert np.abs(diff).max() <= 1 and np.count_nonzero(diff) <= 2
    r = O.decode(w, g["latent"])
    assert np.abs(r.astype(int) - g["recon"].astype(int)).max() <= 1
    np.testing.assert_array_equal(O.histograms(g["latent"]), g["counts"])
    np.testing.assert_allclose(O.hist_entropy(g["latent"]), g["bits"], rtol=0, atol=1e-6)


def test_weights_digest_pinned(manifest, weights_by_init):
    from neural_network_image_compression_amd import weights as W
    assert set(weights_by_init) == set(manifest["weights"])
    for name, w in weights_by_init.items():
        assert W.digest(w) == manifest["weights"][name], name


def test_colour_constants():
    # utils.py:7-9 evaluated in float64 then rounded to fp32 on use
    inv = np.linalg.inv(O.YCBCR_KERNEL_F64).astype(np.float32)
    np.testing.assert_array_equal(inv, O.YCBCR_INV_KERNEL)
    assert O.YCBCR_INV_KERNEL[0, 1] != 0 and abs(O.YCBCR_INV_KERNEL[0, 1]) < 1e-5  # the tiny -7.15e-6 term


def test_colour_forward_is_unfused_fp32():
    x = np.arange(256, dtype=np.uint8)
    rgb = np.stack(np.meshgrid(x, x[::7], x[::13], indexing="ij"), -1).reshape(1, -1, 1, 3)
    y, cb, cr = O.convert_to_colourspace(O.normalise_u8(rgb))
    n = O.normalise_u8(rgb)
    k = O.YCBCR_KERNEL
    for plane, r in ((y, 0), (cb, 1), (cr, 2)):
        a = n[..., 0:1] * k[r, 0]
        b = n[..., 1:2] * k[r, 1]
        c = n[..., 2:3] * k[r, 2]
        ref = ((a + b) + c) + O.YCBCR_OFF[r]
        np.testing.assert_array_equal(plane, ref)
        assert plane.dtype == np.float32


def test_quantise_round_half_even():
    v = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, 0.0, 1.0], np.float32)
    q = O.quantise_u8(v)
    expect = np.round(v * np.float32(255))
    np.testing.assert_array_equal(q, expect.astype(np.uint8))
    assert O.quantise_u8(np.float32([1.0]))[0] == 255


def test_pack_unpack_roundtrip_and_layout():
    rng = np.random.default_rng(3)
    z = rng.integers(0, 256, (2, 3, 5, 96), dtype=np.uint8)
    p = O.pack_latent(z)
    assert p.shape == (2, 12, 40, 3)
    np.testing.assert_array_equal(O.unpack_latent(p), z)
    # raw C-order reinterpretation per plane (utils.py:40)
    np.testing.assert_array_equal(p[1, :, :, 2].ravel(), z[1, :, :, 64:96].ravel())


def test_hist_entropy_edge_cases():
    z = np.zeros((1, 2, 2, 96), np.uint8)
    assert np.all(O.hist_entropy(z) == 0)
    z2 = np.zeros((1, 4, 2, 96), np.uint8)
    for t in range(3):
        z2[0, :, :, 32 * t:32 * t + 32] = np.arange(256, dtype=np.uint8).reshape(4, 2, 32)
    np.testing.assert_allclose(O.hist_entropy(z2).ravel(), [8, 8, 8], atol=1e-5)
    # plane-major order: row p = plane p // N of image p % N
    z3 = np.zeros((2, 1, 1, 96), np.uint8)
    z3[1, ..., 32:64] = np.arange(32)
    h = O.hist_entropy(z3).ravel()
    assert h[3] == pytest.approx(5.0, abs=1e-5) and np.all(np.delete(h, 3) == 0)


def test_reference_decoder_output_size_rounds_up():
    # latent = ceil(H/8); decode returns 8x that
    x = np.zeros((1, 37, 53, 3), np.uint8)
    from neural_network_image_compression_amd import weights as W
    w = W.seeded_weights(1)
    z = O.encode(w, x)
    assert z.shape == (1, 5, 7, 96)
    assert O.decode(w, z).shape == (1, 40, 56, 3)


def test_ms_ssim_properties(golden):
    """MS-SSIM restatement (calc_ssim.py:13): 1 on identical images, symmetric, monotone in noise."""
    x = golden("kodim21_256")["x"]
    assert O.ms_ssim(x, x) == pytest.approx([1.0], abs=1e-12)
    rng = np.random.default_rng(0)
    prev = 1.0
    for amp in (2, 8, 32):
        y = np.clip(x.astype(int) + rng.integers(-amp, amp + 1, x.shape), 0, 255).astype(np.uint8)
        s = O.ms_ssim(x, y)[0]
        assert s < prev
        assert s == pytest.approx(O.ms_ssim(y, x)[0], abs=1e-12)
        prev = s
    # gaussian window: 11 taps, sigma 1.5, normalised
    k = O._fspecial_gauss()
    assert k.shape == (11, 11) and k.sum() == pytest.approx(1.0) and k[5, 5] == k.max()
    with pytest.raises(ValueError):
        O.ms_ssim(x[:, :160, :200], x[:, :160, :200])
    # TF's rule is per scale (ceil halving, each >= 11 px): 161 -> 81 -> 41 -> 21 -> 11
    assert O.ms_ssim_supported(161, 161) and not O.ms_ssim_supported(160, 300)
    assert O.ms_ssim(x[:, :161, :161], x[:, :161, :161]) == pytest.approx([1.0], abs=1e-12)
    from neural_network_image_compression_amd.quality import ms_ssim_supported
    for h in range(150, 180):
        assert ms_ssim_supported(h, 200) == O.ms_ssim_supported(h, 200) == (h >= 161)


def test_power_of_two_weight_scaling_is_exact(golden, weights_spread):
    """The range-guard test's weights (tests/test_gpu_parity.py range_scaled_weights): a layer
    scaled by 2^17 and the next by 2^-17 leave every oracle output bit-identical (leaky is
    positively homogeneous, power-of-two scaling is exact)."""
    from tests.test_gpu_parity import range_scaled_weights
    w = range_scaled_weights(weights_spread)
    g = golden("kodim21_256")
    f = O.encode_f32(w, g["x"])
    np.testing.assert_array_equal(f, g["prequant"])
    np.testing.assert_array_equal(O.decode(w, g["latent"]), g["recon"])
    # the mirror (tests/range_sites.py low_site): the same layers x 2^-17, the next x 2^17, so the
    # scaled layers' activations fall towards the bottom of the f16 range instead of past its top
    from tests.range_sites import _scale_layer
    w = dict(weights_spread)
    _scale_layer(w, "encoderY/", "conv3", -17)
    _scale_layer(w, "decoderCbCr/", "dconv5", -17)
    np.testing.assert_array_equal(O.encode_f32(w, g["x"]), g["prequant"])
    np.testing.assert_array_equal(O.decode(w, g["latent"]), g["recon"])
    a, b = O.encoder_activations(w, g["x"])[0], O.encoder_activations(weights_spread, g["x"])[0]
    np.testing.assert_array_equal(a["conv3"], b["conv3"] * np.float32(2.0 ** -17))
    np.testing.assert_array_equal(a["conv4"], b["conv4"])


def test_float_decoder_check_sees_what_the_u8_check_cannot(weights_spread):
    """tests/test_gpu_parity.py check_recon_f32 on known inputs: one image column 1e-3 off (a
    quarter of a u8 step: a shifted halo column or strip seam) passes check_recon's |delta u8|
    <= 1 and 50 dB and fails the float comparison; the oracle's own fp32-accumulation output,
    the rounding noise a correct fp32 kernel has, passes it."""
    from tests.test_gpu_parity import SHARE_SPREAD, check_recon, check_recon_f32
    z = np.random.default_rng(96).integers(0, 256, (1, 3, 20, 96), dtype=np.uint8)
    rf = O.decode_f32(weights_spread, z)
    assert rf.shape == (1, 24, 160, 3)
    col = 77
    inside = (rf[:, :, col] > 0) & (rf[:, :, col] < 1 - 2e-3)  # the shifted value stays unclipped
    assert inside.mean() >= 0.5
    bad = rf.copy()
    bad[:, :, col][inside] += np.float32(1e-3)
    assert np.abs(bad - rf).max() == pytest.approx(1e-3, rel=1e-3)
    check_recon(O.quantise_u8(bad), O.quantise_u8(rf))
    with pytest.raises(AssertionError, match=f"col {col} "):
        check_recon_f32(bad, O.quantise_u8(bad), rf)
    rf32 = O.decode_f32(weights_spread, z, acc=np.float32)
    worst, share = check_recon_f32(rf32, O.quantise_u8(rf32), rf)
    assert 0 < worst <= 2e-6 and share >= SHARE_SPREAD
    # the u8 output is held to the device's own floats, and to the oracle's away from a .5 boundary
    r = O.quantise_u8(rf)
    flip = r.copy()
    v = rf.astype(np.float64) * 255
    far = (np.abs(v - np.floor(v) - 0.5) > 0.1) & (r < 255)
    at = tuple(np.argwhere(far)[0])
    flip[at] += 1
    with pytest.raises(AssertionError, match="away from a rounding boundary"):
        check_recon_f32(rf, flip, rf)


def test_tile_patches_roundtrip():
    from neural_network_image_compression_amd.rd import tile_patches, untile_patches
    x = np.random.default_rng(0).integers(0, 256, (2, 512, 768, 3), dtype=np.uint8)
    t = tile_patches(x, 256)
    assert t.shape == (12, 256, 256, 3)
    np.testing.assert_array_equal(t[4], x[0, 256:512, 256:512])
    np.testing.assert_array_equal(untile_patches(t, 2, 512, 768), x)
    with pytest.raises(ValueError):
        tile_patches(x[:, :300], 256)


def test_u8_unit_register_division_is_correctly_rounded():
    # csrc u8_unit: b / 255 as r = b * fl(1/255), r += fma(-r, 255, b) * fl(1/255) in fp32 --
    # equal to the correctly rounded b / 255 (the device table c_u8_to_unit, NumPy's
    # astype(f32) / 255) for every byte; exact rational arithmetic for each rounding step
    from fractions import Fraction as F

    def r32(x):
        c = np.float32(float(x))
        cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
        return min(cands, key=lambda v: (abs(F(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))

    c = np.float32(0.0039215688593685627)
    assert c == r32(F(1, 255))
    for b in range(256):
        r = r32(F(b) * F(float(c)))
        e = r32(F(b) - F(float(r)) * 255)
        q = r32(F(float(e)) * F(float(c)) + F(float(r)))
        assert q == np.float32(b) / np.float32(255), b
