"""CPU checks of the .nic container's version 3: the pure-Python reference (tests/rans3_ref.py) on
the golden latents, a hand-computed file, the degenerate context prior that reproduces version 2,
the exact tie, prior.ContextPrior and the .nicc file, and the host-only entry points
nic_rans_cprior_check / nic_rans3_inspect / nic_rans3_bound plus the argument checks of the device
entry points (no GPU calls here)."""
import ctypes
import glob
import os
import struct

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from neural_network_image_compression_amd import bitstream as B
from neural_network_image_compression_amd.prior import ContextPrior
from tests import rans2_ref as R2
from tests import rans3_ref as R3
from tests import rans_ref as R
from tests.conftest import GOLDEN, load_case
from tests.nic_bad_files import as_file, corruptions, inspector_refuses

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
SEG_PIXELS = (1, 7, 32, 4096)


@pytest.fixture(scope="module")
def fitted():
    """A context prior fitted on the trained 32x32 latent and the four trained 16x16 latents."""
    zs = list(load_case("kodim21_256_trained")["latent"]) + list(load_case("imagenet4_trained")["latent"])
    return R3.fit_context_prior(zs)


def inspect3(data):
    v = [ctypes.c_int(-1) for _ in range(5)]
    pid = ctypes.c_uint32(0)
    buf = np.frombuffer(data, np.uint8)
    rc = _lib.lib().nic_rans3_inspect(buf.ctypes.data, len(data), *[ctypes.byref(t) for t in v], ctypes.byref(pid))
    return rc, tuple(t.value for t in v) + (pid.value,)


@pytest.mark.parametrize("case", CASES)
def test_reference_round_trips(case, fitted):
    latents = load_case(case)["latent"]
    for kind, cprior in (("fitted", fitted), ("uniform", R3.uniform_context_prior())):
        pid = R3.prior_id(cprior)
        for i, z in enumerate(latents):
            h8, w8 = z.shape[:2]
            for sp in SEG_PIXELS:
                data = R3.write_file(z, cprior, sp)
                np.testing.assert_array_equal(R3.read_file(data, cprior), z)
                assert inspect3(data) == (_lib.NIC_OK, (h8, w8, sp, 8 * h8, 8 * w8, pid))
                assert B.nic3_inspect(data) == (h8, w8, sp, 8 * h8, 8 * w8, pid)
                print(f"{case}[{i}] {kind} seg_pixels {sp}: {len(data)} B, own-table channels {sum(R3.parse_file(data)['mask'])}")
    with pytest.raises(ValueError, match="prior"):
        R3.read_file(data, fitted)  # data was written under the uniform context prior


def _hand_prior():
    """Anchor 10 everywhere; row 0 uniform, row 1 favours symbol 13, row 2 favours symbol 10."""
    row0 = [16] * 256
    row1 = [15] * 256
    row1[13] += 256
    row2 = [14] * 256
    row2[10] += 512
    assert sum(row0) == sum(row1) == sum(row2) == 4096
    return [10] * 96, [[row0, row1, row2] for _ in range(96)]


def _rans_by_hand(steps):
    """steps: (freq, start) of every symbol in coding order (first symbol first) -> the segment."""
    out, x = [], 1 << 23
    for fr, st in reversed(steps):
        while x >= fr << 19:
            out.append(x & 255)
            x >>= 8
        x = ((x // fr) << 12) + (x % fr) + st
    return bytes(reversed(out + [(x >> (8 * i)) & 255 for i in range(4)]))


def test_hand_computed_contexts():
    cprior = _hand_prior()
    z = np.zeros((1, 3, 96), np.uint8)
    z[0, 0], z[0, 1], z[0, 2] = 11, 13, 10  # |11 - 10| = 1: pixel 1 in context 1; |13 - 10| = 3: pixel 2 in context 2
    pid = struct.pack("<I", R3.prior_id(cprior))
    head = lambda sp: b"NICR" + struct.pack("<BBHIIII", 3, 12, sp, 1, 3, 8, 24) + pid + bytes(12)  # noqa: E731
    # seg_pixels 3: one segment, the three contexts hit in turn; no channel keeps a table (three
    # symbols under the prior cost at most 3 x 8 bits, a table of three entries 80)
    seg = _rans_by_hand([(16, 11 * 16)] * 96 + [(15 + 256, 13 * 15)] * 96 + [(14 + 512, 10 * 14)] * 96)
    want = head(3) + struct.pack("<I", len(seg)) + seg
    assert R3.write_file(z, cprior, 3) == want
    np.testing.assert_array_equal(R3.read_file(want, cprior), z)
    # seg_pixels 1: every pixel opens a segment, so everything is context 0
    segs = [_rans_by_hand([(16, s * 16)] * 96) for s in (11, 13, 10)]
    want1 = head(1) + b"".join(struct.pack("<I", len(s)) for s in segs) + b"".join(segs)
    got1 = R3.write_file(z, cprior, 1)
    assert got1 == want1 and len(got1) != len(want)
    # ... which is the file coded with rows 1 and 2 replaced by row 0, but for that prior's id
    flat = (cprior[0], [[rows[0]] * 3 for rows in cprior[1]])
    other = R3.write_file(z, flat, 1)
    assert other[:24] == got1[:24] and other[28:] == got1[28:] and other[24:28] == struct.pack("<I", R3.prior_id(flat))
    assert inspect3(want)[0] == inspect3(want1)[0] == _lib.NIC_OK


def test_three_equal_rows_reproduce_version_2(golden):
    P = R2.fit_prior(golden("imagenet4_trained")["latent"])
    cprior = R3.replicate(P)
    for case, size in (("kodim21_256_trained", None), ("odd37x53", (37, 53))):
        z = golden(case)["latent"][0]
        for sp in (7, 32):
            v2, v3 = R2.write_file(z, P, sp, size), R3.write_file(z, cprior, sp, size)
            assert len(v2) == len(v3)
            diff = [i for i in range(len(v2)) if v2[i] != v3[i]]
            assert set(diff) <= {4, 24, 25, 26, 27} and 4 in diff, (case, sp, diff[:10])
            assert v3[4] == 3 and v3[24:28] == struct.pack("<I", R3.prior_id(cprior))
    # the uniform context prior: the version-2 figure of DESIGN section 12
    data = R3.write_file(golden("kodim21_256_trained")["latent"][0], R3.uniform_context_prior())
    assert len(data) == 5466


def test_exact_tie_goes_to_the_prior():
    # as tests/test_gpu_rans2.py builds it: a constant channel's table costs 8 (1 + 3) = 32 bits and
    # 32 pixels at prior freq 2048 cost 32 x 1 bit; here the three context rows all carry that freq
    anchors, freqs = R3.uniform_context_prior()
    freqs[0] = [[2048 - 254] + [1] * 6 + [2048] + [1] * 248 for _ in range(3)]
    cprior = (anchors, freqs)
    rng = np.random.default_rng(3)
    for (h8, w8), own in (((4, 8), False), ((3, 11), True)):
        z = rng.integers(0, 256, (h8, w8, 96), dtype=np.uint8)
        z[..., 0] = 7
        counts = R3.context_counts(z, anchors, 32)
        assert counts[0].sum() == h8 * w8 and counts[0][0][7] == -(-h8 * w8 // 32)  # a segment's first pixel: context 0
        assert R3.choose(counts[0], freqs[0])[0] is own
        data = R3.write_file(z, cprior)
        assert R3.parse_file(data, cprior)["mask"][0] is own
        np.testing.assert_array_equal(R3.read_file(data, cprior), z)


def _check(anchors, freqs):
    a, f = np.ascontiguousarray(anchors, np.uint8), np.ascontiguousarray(freqs, np.uint16)
    pid = ctypes.c_uint32(0)
    return _lib.lib().nic_rans_cprior_check(a.ctypes.data, f.ctypes.data, ctypes.byref(pid)), pid.value


def test_context_prior_and_the_nicc_file(fitted, tmp_path):
    for cprior in (R3.uniform_context_prior(), fitted):
        assert _check(*cprior) == (_lib.NIC_OK, R3.prior_id(cprior))
        p = ContextPrior(*cprior)
        assert p.id == R3.prior_id(cprior) and p.to_bytes() == R3.write_nicc(cprior) and len(p.to_bytes()) == 147568
        p.save(str(tmp_path / "p.nicc"))
        q = ContextPrior.load(str(tmp_path / "p.nicc"))
        assert q == p and q.id == p.id
        assert R3.read_nicc((tmp_path / "p.nicc").read_bytes()) == (list(cprior[0]), [[list(r) for r in c] for c in cprior[1]])
    # the anchors are part of the id
    a2 = list(fitted[0])
    a2[5] ^= 1
    assert ContextPrior(a2, fitted[1]).id != ContextPrior(*fitted).id and ContextPrior(a2, fitted[1]) != ContextPrior(*fitted)
    anchors, good = R3.uniform_context_prior()
    good = np.array(good, np.uint16)
    bad = {}
    bad["a zero freq"] = good.copy()
    bad["a zero freq"][17, 2, 3], bad["a zero freq"][17, 2, 4] = 0, 32
    bad["a row summing to 4095"] = good.copy()
    bad["a row summing to 4095"][17, 2, 3] = 15
    bad["a freq of 4097"] = good.copy()
    bad["a freq of 4097"][17, 2, 3] = 4097
    for name, f in bad.items():
        rc, _ = _check(anchors, f)
        assert rc == _lib.NIC_ECORRUPT, name
        assert "channel 17 context 2" in _lib.last_error(), name
        with pytest.raises(ValueError, match="channel 17 context 2"):
            ContextPrior(anchors, f)
    assert _lib.lib().nic_rans_cprior_check(None, None, None) == _lib.NIC_EINVAL
    with pytest.raises(ValueError):
        ContextPrior([0] * 95, good)
    with pytest.raises(ValueError):
        ContextPrior([256] + [0] * 95, good)
    # the .nicc reader refuses a damaged file
    data = bytearray(R3.write_nicc(fitted))
    at_freq = 16 + 96 + 2 * ((17 * 3 + 2) * 256 + 3)
    for at, what in ((0, "magic"), (4, "version"), (8, "prior_id"), (12, "contexts"), (13, "reserved"), (15, "reserved"),
                     (at_freq, "freq"), (16 + 40, "anchor")):
        d = bytearray(data)
        d[at] ^= 1
        with pytest.raises(ValueError):
            ContextPrior.from_bytes(bytes(d))
        with pytest.raises(ValueError):
            R3.read_nicc(bytes(d))
    for d in (data[:-1], data + b"\0", data[:100]):
        with pytest.raises(ValueError):
            ContextPrior.from_bytes(bytes(d))


def test_inspect_rejects_corrupt_files(golden):
    z = golden("kodim21_256_trained")["latent"][0]
    cprior = R3.fit_context_prior(golden("imagenet4_trained")["latent"])
    data = R3.write_file(z, cprior)
    assert 0 < sum(R3.parse_file(data)["mask"]) < 96
    bad = corruptions(3, data, lambda sp: R3.write_file(z, cprior, sp))
    assert {"version 1", "version 2", "version 4"} <= set(bad) and "version 3" not in bad
    assert len(bad) >= 45
    buf_of = lambda d: np.frombuffer(d, np.uint8).ctypes.data  # noqa: E731
    for name, (d, size, _) in bad.items():
        rc = _lib.lib().nic_rans3_inspect(buf_of(d), size, None, None, None, None, None, None)
        if not inspector_refuses(name):
            assert rc == _lib.NIC_OK, name
            continue
        assert rc == _lib.NIC_ECORRUPT, name
        assert "nic_rans3_inspect" in _lib.last_error(), name
        with pytest.raises(ValueError):
            B.nic3_inspect(as_file(d, size))
        with pytest.raises(ValueError):
            R3.parse_file(as_file(d, size))
    # version-1 and version-2 files are not version-3 files, and the other way round
    v1 = R.write_file(z)
    v2 = R2.write_file(z, R2.uniform_prior())
    assert inspect3(v1)[0] == _lib.NIC_ECORRUPT and "version 1" in _lib.last_error()
    assert inspect3(v2)[0] == _lib.NIC_ECORRUPT and "version 2" in _lib.last_error()
    for d in (v1, v2):
        with pytest.raises(ValueError):
            R3.parse_file(d)
    buf = np.frombuffer(data, np.uint8)
    assert _lib.lib().nic_rans_inspect(buf.ctypes.data, len(data), None, None, None) == _lib.NIC_ECORRUPT
    assert "version 3" in _lib.last_error()
    assert _lib.lib().nic_rans2_inspect(buf.ctypes.data, len(data), None, None, None, None, None, None) == _lib.NIC_ECORRUPT
    assert "version 3" in _lib.last_error()
    for f in (B.nic_inspect, B.nic2_inspect, R.parse_file, R2.parse_file):
        with pytest.raises(ValueError):
            f(data)
    # the outputs are optional
    assert _lib.lib().nic_rans3_inspect(buf.ctypes.data, len(data), None, None, None, None, None, None) == _lib.NIC_OK


def test_bound_is_the_version_2_bound():
    L = _lib.lib()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for h8, w8, sp in ((1, 1, 32), (5, 7, 32), (32, 32, 1), (32, 32, 4096), (270, 480, 32)):
        assert L.nic_rans2_bound(h8, w8, sp, ctypes.byref(a)) == _lib.NIC_OK
        assert L.nic_rans3_bound(h8, w8, sp, ctypes.byref(b)) == _lib.NIC_OK
        assert b.value == a.value
    assert L.nic_rans3_bound(1, 1, 32, None) == _lib.NIC_EINVAL
    assert L.nic_rans3_bound(0, 1, 32, ctypes.byref(b)) == _lib.NIC_ESHAPE
    assert L.nic_rans3_bound(1, 1, 65536, ctypes.byref(b)) == _lib.NIC_ESHAPE


def test_entry_points_validate_without_a_gpu():
    L = _lib.lib()
    assert L.nic_version() >= 600 and _lib.NIC_ENOPRIOR == -8
    assert L.nic_rans3_inspect(None, 100, None, None, None, None, None, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()
    # device entry points: shape, empty batch, then NULL, all before any HIP call (the prior is
    # looked at last: NIC_ENOPRIOR needs a context, tests/test_gpu_rans3.py)
    big = 1 << 20
    assert L.nic_rans3_encode(None, None, 1, 4, 4, 32, 32, 32, None, big, None, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()
    assert L.nic_rans3_encode(None, None, 1, 0, 4, 32, 32, 32, None, big, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans3_encode(None, None, -1, 4, 4, 32, 32, 32, None, big, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans3_encode(None, None, 1, 4, 4, 32, 32, 0, None, big, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans3_encode(None, None, 1, 4, 4, 33, 32, 32, None, big, None, None) == _lib.NIC_ESHAPE  # 33 rows: h8 = 5
    assert L.nic_rans3_encode(None, None, 1, 4, 4, 32, 24, 32, None, big, None, None) == _lib.NIC_ESHAPE  # 24 columns: w8 = 3
    assert L.nic_rans3_encode(None, None, 1, 4, 4, 25, 31, 32, None, big, None, None) == _lib.NIC_EINVAL  # 25 x 31 is 4 x 4
    assert L.nic_rans3_encode(None, None, 0, 4, 4, 32, 32, 32, None, 0, None, None) == _lib.NIC_OK  # empty batch
    assert L.nic_rans3_decode(None, None, big, None, 1, 4, 4, None, None, None) == _lib.NIC_EINVAL
    assert L.nic_rans3_decode(None, None, big, None, 1, 4, 0, None, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans3_decode(None, None, 0, None, 0, 4, 4, None, None, None) == _lib.NIC_OK
    assert L.nic_rans3_reserve(None, 1, 4, 4, 32) == _lib.NIC_EINVAL
    assert L.nic_rans3_reserve(None, 1, 4, 4, 70000) == _lib.NIC_ESHAPE
    assert L.nic_rans3_reserve(None, 0, 4, 4, 32) == _lib.NIC_OK
    assert L.nic_rans_cprior_count(None, None, 1, 4, 4, 32, None, None, None) == _lib.NIC_EINVAL
    assert L.nic_rans_cprior_count(None, None, 1, 4, 0, 32, None, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans_cprior_count(None, None, 1, 4, 4, 0, None, None, None) == _lib.NIC_ESHAPE
    assert L.nic_rans_cprior_count(None, None, 0, 4, 4, 32, None, None, None) == _lib.NIC_OK
    assert L.nic_rans_cprior_build(None, None, None, None) == _lib.NIC_EINVAL
    assert L.nic_rans_cprior_set(None, None, None, None) == _lib.NIC_EINVAL
