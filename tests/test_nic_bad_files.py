"""CPU checks of the damaged-file catalogue (tests/nic_bad_files.py) on its small bases: the host
inspectors and the strict reference readers refuse every case their contract covers, and the lenient
reader model (tests/rans_read_model.py), which supplies the device tests' expected statuses
(tests/test_gpu_rans_malformed.py), agrees with the masks the catalogue takes from nic.h."""
import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from tests import nic_bad_files as NB
from tests import rans2_ref as R2
from tests import rans3_ref as R3
from tests import rans_read_model as RM
from tests import rans_ref as R

KEYS = sorted(NB.bases(), key=str)


def _inspect(ver, d, size):
    """nic_rans*_inspect on the slot's bytes with the case's size (which may be 0 or negative)."""
    buf = np.frombuffer(d, np.uint8)
    fn = getattr(_lib.lib(), {1: "nic_rans_inspect", 2: "nic_rans2_inspect", 3: "nic_rans3_inspect"}[ver])
    return fn(buf.ctypes.data, size, *([None] * (3 if ver == 1 else 6)))


def _parse(b, d):
    return {1: lambda: R.parse_file(d), 2: lambda: R2.parse_file(d, b["prior"]), 3: lambda: R3.parse_file(d, b["prior"])}[b["ver"]]()


def _read(b, d):
    return {1: lambda: R.read_file(d), 2: lambda: R2.read_file(d, b["prior"]), 3: lambda: R3.read_file(d, b["prior"])}[b["ver"]]()


def test_the_catalogue_holds_every_class():
    names = {k: set(NB.bases()[k]["cases"]) for k in KEYS}
    for key in (("v1 5x7", 3), ("v1 5x7", 32), ("v2 9x11", 3), ("v3 9x11", 32)):
        have = names[key]
        for must in ("a freq of 0, the others still summing to 4096", "one entry of freq 4097", "two entries of 3000 and 3000",
                     "freqs sum to 4097", "n-1 raised by one", "n-1 lowered by one", "n-1 255 on the last table, the file ends inside it",
                     "freqs sum to 4095", "descending symbols", "equal symbols", "size 0", "size -1", "segment length raised by one",
                     "a segment length of 0", "a segment length of 0xFFFFFFFF", "every segment length 0xFFFFFFFF", "seg_pixels 65535",
                     "one byte appended", "last segment length raised by one", "bad magic", "seg_pixels 0"):
            assert must in have, (key, must)
        assert sum(1 for n in have if n.startswith("cut at")) >= 10
        if key[0] != "v1 5x7":
            for must in ("H one row too many for h8", "a mask bit set with no table behind it", "a mask bit cleared in front of its table",
                         "all twelve mask bytes 0xFF", "a foreign prior_id"):
                assert must in have, (key, must)
    assert {"length of segment 255 raised by one", "length of segment 256 raised by one"} <= names[("v1 17x16", 1)]
    for key in KEYS:  # the crafted latent's files: at least two own tables and a prior channel
        b = NB.bases()[key]
        if b["ver"] != 1:
            assert 2 <= len(NB.layout(b["ver"], b["data"])["tables"]) < 96


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_inspector_and_reference_refuse(key):
    b = NB.bases()[key]
    assert _inspect(b["ver"], b["data"], len(b["data"])) == _lib.NIC_OK
    _parse(b, b["data"])
    for name, (d, size, _) in b["cases"].items():
        if not NB.inspector_refuses(name):
            if name in NB.LEGAL | NB.DECODE_ONLY:
                assert _inspect(b["ver"], d, size) == _lib.NIC_OK, name
            if name in NB.DECODE_ONLY:
                with pytest.raises(ValueError):
                    _read(b, d)
            continue
        assert _inspect(b["ver"], d, size) == _lib.NIC_ECORRUPT, name
        with pytest.raises(ValueError):
            _parse(b, NB.as_file(d, size))


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_model_reads_good_files_and_stays_inside_the_masks(key):
    b = NB.bases()[key]
    status, z = RM.read(b["ver"], b["data"], len(b["data"]), b["h8"], b["w8"], b["prior"])
    assert status == 0
    np.testing.assert_array_equal(z, b["latent"])
    # the same file in a longer slot, and with a size past the slot
    slot = b["data"] + b"\xa5" * 37
    assert RM.read(b["ver"], slot, len(b["data"]), b["h8"], b["w8"], b["prior"])[0] == 0
    assert RM.read(b["ver"], b["data"], len(b["data"]) + 1000, b["h8"], b["w8"], b["prior"], stride=len(b["data"]))[0] == 0
    model = NB.model_of(key)
    for name, (d, size, expected) in b["cases"].items():
        status, z = model[name]
        print(f"{key} {name}: model status {status}")
        assert NB.within(status, name, expected), (name, status, expected)
        # no case but the bookkeeping class and the legal file may be predicted clean
        assert (status == 0) == (name in NB.BOOKKEEPING | NB.LEGAL), (name, status)
        if status == 0:
            np.testing.assert_array_equal(z, b["latent"])


def test_lenient_row_resolves_every_slot():
    rng = np.random.default_rng(5)
    tables = [[(3, 4096)], [(0, 0), (9, 4096)], [(7, 5000)], [(1, 3000), (2, 3000)], [(5, 10), (4, 4086)], [(5, 10), (5, 4086)],
              [(0, 65535), (255, 65535)], [(255, 1)], [(s, 16) for s in range(256)], [(s, 17) for s in range(256)]]
    tables += [[(int(s), int(f)) for s, f in zip(rng.integers(0, 256, n), rng.integers(0, 6000, n))] for n in (1, 2, 17, 256)]
    for ent in tables:
        start, broken = RM.lenient_row(ent)
        assert len(start) == 257 and start[0] == 0 and start[256] == 4096 and all(a <= b for a, b in zip(start, start[1:])), ent
        strict = (all(a[0] < b[0] for a, b in zip(ent, ent[1:])) and all(1 <= f <= 4096 for _, f in ent)
                  and sum(f for _, f in ent) == 4096)
        assert broken == (not strict), ent
