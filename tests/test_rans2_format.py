"""CPU checks of the .nic container's version 2: the pure-Python reference (tests/rans2_ref.py) on
the golden latents under three priors, the size claims that motivate the prior, and the host-only
entry points nic_rans_cost_table / nic_rans_prior_check / nic_rans2_inspect / nic_rans2_bound plus
the argument checks of the device entry points (no GPU calls here)."""
import ctypes
import glob
import os

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from neural_network_image_compression_amd import bitstream as B
from neural_network_image_compression_amd.prior import Prior
from tests import rans2_ref as R2
from tests import rans_ref as R
from tests.conftest import GOLDEN, load_case
from tests.nic_bad_files import as_file, corruptions, inspector_refuses

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
PRIORS = ("uniform", "self", "other")


@pytest.fixture(scope="module")
def priors():
    """(case, kind) -> prior: uniform, fitted on the case's own latents, or fitted on another
    codec's latents (the glorot codec's for a trained case, the trained coef-0.01 codec's else)."""
    cache = {}

    def fitted(case):
        if case not in cache:
            cache[case] = R2.fit_prior(load_case(case)["latent"])
        return cache[case]

    def get(case, kind):
        if kind == "uniform":
            return R2.uniform_prior()
        if kind == "self":
            return fitted(case)
        return fitted("kodim21_glorot" if "trained" in case else "kodim21_256_trained")

    return get


@pytest.fixture(scope="module")
def v1_files():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = [R.write_file(z) for z in load_case(case)["latent"]]
        return cache[case]

    return get


def inspect2(data):
    v = [ctypes.c_int(-1) for _ in range(5)]
    pid = ctypes.c_uint32(0)
    buf = np.frombuffer(data, np.uint8)
    rc = _lib.lib().nic_rans2_inspect(buf.ctypes.data, len(data), *[ctypes.byref(t) for t in v], ctypes.byref(pid))
    return rc, tuple(t.value for t in v) + (pid.value,)


@pytest.mark.parametrize("case", CASES)
def test_reference_round_trips_under_three_priors(case, priors, v1_files):
    latents = load_case(case)["latent"]
    for kind in PRIORS:
        prior = priors(case, kind)
        pid = R2.prior_id(prior)
        for i, z in enumerate(latents):
            data = R2.write_file(z, prior)
            np.testing.assert_array_equal(R2.read_file(data, prior), z)
            info = R2.parse_file(data, prior)
            nseg, v1 = len(info["seg_lengths"]), v1_files(case)[i]
            print(f"{case}[{i}] {kind}: v1 {len(v1)} v2 {len(data)} own-table channels {sum(info['mask'])}")
            # a bad prior costs the 24 header bytes (every channel falls back to its own table),
            # plus a byte of segment granularity where some channels switch
            assert len(data) <= len(v1) + 24 + nseg
            # the library's inspector agrees on every field
            h8, w8 = z.shape[:2]
            assert inspect2(data) == (_lib.NIC_OK, (h8, w8, 32, 8 * h8, 8 * w8, pid))
            assert B.nic2_inspect(data) == (h8, w8, 32, 8 * h8, 8 * w8, pid)
            # and the version-1 inspector refuses the file
            buf = np.frombuffer(data, np.uint8)
            assert _lib.lib().nic_rans_inspect(buf.ctypes.data, len(data), None, None, None) == _lib.NIC_ECORRUPT
    with pytest.raises(ValueError, match="prior"):
        R2.read_file(data, R2.fit_prior([latents[0][:1]]))


def test_true_image_size_and_other_segment_sizes(golden):
    z = golden("odd37x53")["latent"][0]
    prior = R2.uniform_prior()
    for sp in (1, 7, 4096):
        data = R2.write_file(z, prior, sp, size=(37, 53))
        assert inspect2(data) == (_lib.NIC_OK, (5, 7, sp, 37, 53, R2.prior_id(prior)))
        np.testing.assert_array_equal(R2.read_file(data, prior), z)
    # the outputs are optional
    buf = np.frombuffer(data, np.uint8)
    assert _lib.lib().nic_rans2_inspect(buf.ctypes.data, len(data), None, None, None, None, None, None) == _lib.NIC_OK


def test_imagenet_files_shrink_under_a_small_prior(golden, v1_files):
    prior = R2.fit_prior(golden("kodim21_256_trained")["latent"])
    v1 = [len(d) for d in v1_files("imagenet4_trained")]
    v2 = [len(R2.write_file(z, prior)) for z in golden("imagenet4_trained")["latent"]]
    print(f"imagenet4_trained: v1 {v1} v2 {v2} ratio {sum(v2) / sum(v1):.3f}")
    assert all(b < a for a, b in zip(v1, v2))
    assert sum(v2) <= 0.80 * sum(v1)


def test_tiny_image_under_the_uniform_prior_is_under_half(golden, v1_files):
    v1, = v1_files("odd37x53")
    v2 = R2.write_file(golden("odd37x53")["latent"][0], R2.uniform_prior(), size=(37, 53))
    print(f"odd37x53: v1 {len(v1)} v2 {len(v2)}")
    assert 2 * len(v2) < len(v1)


def test_prior_normalisation_on_hard_histograms():
    hard = {
        "empty": [0] * 256,
        "one symbol": [0] * 255 + [5184],
        "255 singletons beside one dominant symbol": [1] * 255 + [10 ** 6],
        "all equal": [20] * 256,
        "128 rare and 128 equal": [1] * 128 + [1000] * 128,
        "counts near 2^52": [0] * 254 + [2 ** 51, 2 ** 51 - 1],
    }
    for name, counts in hard.items():
        f = R2.normalise_prior(counts)
        assert sum(f) == 4096 and min(f) >= 1 and max(f) <= 4096, name
    assert R2.normalise_prior([0] * 256) == [16] * 256
    assert R2.normalise_prior([1] * 255 + [10 ** 6])[255] == 4096 - 255


def test_cost_table_is_the_reference_table():
    out = np.full(4097, 0xFFFFFFFF, np.uint32)
    assert _lib.lib().nic_rans_cost_table(out.ctypes.data) == _lib.NIC_OK
    assert out.tolist() == R2.COST16
    assert R2.COST16[0] == 0 and R2.COST16[1] == 12 << 16 and R2.COST16[4096] == 0 and R2.COST16[2048] == 1 << 16
    assert _lib.lib().nic_rans_cost_table(None) == _lib.NIC_EINVAL


def _check(freqs):
    a = np.ascontiguousarray(freqs, np.uint16)
    pid = ctypes.c_uint32(0)
    return _lib.lib().nic_rans_prior_check(a.ctypes.data, ctypes.byref(pid)), pid.value


def test_prior_check_and_the_nicp_file(golden, tmp_path):
    for prior in (R2.uniform_prior(), R2.fit_prior(golden("kodim21_256_trained")["latent"]),
                  R2.fit_prior(golden("kodim21_glorot")["latent"])):
        assert _check(prior) == (_lib.NIC_OK, R2.prior_id(prior))
        p = Prior(prior)
        assert p.id == R2.prior_id(prior) and p.to_bytes() == R2.write_nicp(prior) and len(p.to_bytes()) == 49168
        p.save(str(tmp_path / "p.nicp"))
        q = Prior.load(str(tmp_path / "p.nicp"))
        assert q == p and q.id == p.id and R2.read_nicp((tmp_path / "p.nicp").read_bytes()) == prior
    good = np.array(R2.uniform_prior(), np.uint16)
    bad = {}
    bad["a zero freq"] = good.copy()
    bad["a zero freq"][17, 3], bad["a zero freq"][17, 4] = 0, 32
    bad["a row summing to 4095"] = good.copy()
    bad["a row summing to 4095"][17, 3] = 15
    bad["a freq above 4096"] = good.copy()
    bad["a freq above 4096"][17, 3] = 4097
    for name, a in bad.items():
        rc, _ = _check(a)
        assert rc == _lib.NIC_ECORRUPT, name
        assert "channel 17" in _lib.last_error(), name
        with pytest.raises(ValueError, match="channel 17"):
            Prior(a)
    assert _lib.lib().nic_rans_prior_check(None, None) == _lib.NIC_EINVAL
    # the .nicp reader refuses a damaged file
    data = bytearray(R2.write_nicp(R2.uniform_prior()))
    for at, what in ((0, "magic"), (4, "version"), (8, "prior_id"), (12, "reserved word"), (16 + 2 * (17 * 256 + 3), "freq")):
        d = bytearray(data)
        d[at] ^= 1
        with pytest.raises(ValueError):
            Prior.from_bytes(bytes(d))
    with pytest.raises(ValueError):
        Prior.from_bytes(bytes(data[:-1]))


def _inspect_sized(d, size):
    buf = np.frombuffer(d, np.uint8)
    return _lib.lib().nic_rans2_inspect(buf.ctypes.data, size, None, None, None, None, None, None)


def test_inspect_rejects_corrupt_files(golden, v1_files):
    z = golden("kodim21_256_trained")["latent"][0]
    prior = R2.fit_prior(golden("imagenet4_trained")["latent"])
    data = R2.write_file(z, prior)
    assert 0 < sum(R2.parse_file(data)["mask"]) < 96
    bad = corruptions(2, data, lambda sp: R2.write_file(z, prior, sp))
    for must in ("bad magic", "version 1", "version 3", "probability bits 11", "truncated by one byte", "one byte appended",
                 "segment length raised by one", "freqs sum to 4095", "descending symbols", "equal symbols", "seg_pixels 0", "h8 0",
                 "header only", "shorter than the header", "a mask bit set with no table behind it",
                 "a mask bit cleared in front of its table", "H one row too many for h8", "H too small for h8", "W 0"):
        assert must in bad
    assert len(bad) >= 45
    for name, (d, size, _) in bad.items():
        if not inspector_refuses(name):
            assert _inspect_sized(d, size) == _lib.NIC_OK, name
            continue
        assert _inspect_sized(d, size) == _lib.NIC_ECORRUPT, name
        assert "nic_rans2_inspect" in _lib.last_error(), name
        with pytest.raises(ValueError):
            B.nic2_inspect(as_file(d, size))
        with pytest.raises(ValueError):
            R2.parse_file(as_file(d, size))
    # a version-1 file is not a version-2 file, and the other way round
    v1, = v1_files("kodim21_256_trained")
    assert inspect2(v1)[0] == _lib.NIC_ECORRUPT and "version 1" in _lib.last_error()
    buf = np.frombuffer(data, np.uint8)
    assert _lib.lib().nic_rans_inspect(buf.ctypes.data, len(data), None, None, None) == _lib.NIC_ECORRUPT
    assert "version 2" in _lib.last_error()
    with pytest.raises(ValueError):
        B.nic_inspect(data)


def test_bound_is_the_version_1_bound_plus_24():
    L = _lib.lib()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for h8, w8, sp in ((1, 1, 32), (5, 7, 32), (32, 32, 1), (32, 32, 4096), (270, 480, 32)):
        assert L.nic_rans_bound(h8, w8, sp, ctypes.byref(a)) == _lib.NIC_OK
        assert L.nic_rans2_bound(h8, w8, sp, ctypes.byref(b)) == _lib.NIC_OK
        assert b.value == a.value + 24
    assert L.nic_rans2_bound(1, 1, 32, None) == _lib.NIC_EINVAL
    assert L.nic_rans2_bound(0, 1, 32, ctypes.byref(b)) == _lib.NIC_ESHAPE
    assert L.nic_rans2_bound(1, 1, 65536, ctypes.byref(b)) == _lib.NIC_ESHAPE


def test_entry_points_validate_without_a_gpu():
    L = _lib.lib()
    assert L.nic_version() >= 500 and _lib.NIC_ENOPRIOR == -8
    assert L.nic_rans2_inspect(None, 100, None, None, None, None, None, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()
    # device entry points: shape, empty batch, then NULL, all before any HIP call (the prior is
    # looked at last: NIC_ENOPRIOR needs a context, tests/test_gpu_rans2.py)
    big = 1 << 20
    assert L.nic_rans2_encode(None, None, 1, 4, 4, 32, 32, 32, None, big, None, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()
    assert L.nic_rans2_encode(None, None, 1, 0, 4, 32, 32, 32, None, big, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans2_encode(None, None, -1, 4, 4, 32, 32, 32, None, big, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans2_encode(None, None, 1, 4, 4, 32, 32, 0, None, big, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans2_encode(None, None, 1, 4, 4, 33, 32, 32, None, big, None, None) == _lib.NIC_ESHAPE  # 33 rows: h8 = 5
    assert L.nic_rans2_encode(None, None, 1, 4, 4, 32, 24, 32, None, big, None, None) == _lib.NIC_ESHAPE  # 24 columns: w8 = 3
    assert L.nic_rans2_encode(None, None, 1, 4, 4, 25, 31, 32, None, big, None, None) == _lib.NIC_EINVAL  # 25 x 31 is 4 x 4
    assert L.nic_rans2_encode(None, None, 0, 4, 4, 32, 32, 32, None, 0, None, None) == _lib.NIC_OK  # empty batch
    assert L.nic_rans2_decode(None, None, big, None, 1, 4, 4, None, None, None) == _lib.NIC_EINVAL
    assert L.nic_rans2_decode(None, None, big, None, 1, 4, 0, None, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans2_decode(None, None, 0, None, 0, 4, 4, None, None, None) == _lib.NIC_OK
    assert L.nic_rans2_reserve(None, 1, 4, 4, 32) == _lib.NIC_EINVAL
    assert L.nic_rans2_reserve(None, 1, 4, 4, 70000) == _lib.NIC_ESHAPE
    assert L.nic_rans2_reserve(None, 0, 4, 4, 32) == _lib.NIC_OK
    assert L.nic_rans_prior_count(None, None, 1, 4, 4, None, None) == _lib.NIC_EINVAL
    assert L.nic_rans_prior_count(None, None, 1, 4, 0, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans_prior_count(None, None, 0, 4, 4, None, None) == _lib.NIC_OK
    assert L.nic_rans_prior_build(None, None, None, None) == _lib.NIC_EINVAL
    assert L.nic_rans_prior_set(None, None, None) == _lib.NIC_EINVAL
