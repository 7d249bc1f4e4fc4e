"""One catalogue of damaged .nic files for every reader of the format: the host inspectors
(tests/test_rans_format.py, test_rans2_format.py, test_rans3_format.py), the lenient reader model
(tests/rans_read_model.py, tests/test_nic_bad_files.py) and the device reader
(tests/test_gpu_rans_malformed.py).  Nothing here touches the library.

corruptions(ver, data) makes, from one well-formed file, name -> (bytes, size, (must, may)):
the bytes of the slot, the size to pass for it (a truncation passes a smaller size with the
original bytes still behind it), and what nic.h's status word may be for it on the device: every bit
of `must` is set, no bit outside `may` is, and the status is non-zero unless the name is in
BOOKKEEPING or LEGAL.  The masks come from nic.h's text, never from a reader's output.
"""
import functools
import struct

import numpy as np

from tests import rans2_ref as R2
from tests import rans3_ref as R3
from tests import rans_ref as R

SEG, HDR, TAB, PRIOR = 1, 2, 4, 8  # nic.h's status bits 0 to 3
HEADER = {1: 16, 2: 40, 3: 40}

# the inspector refuses these, but nic.h gives the device no bit for them: header + tables + segment
# table + sum of lengths == size is the inspector's check alone, and the device decodes them cleanly
BOOKKEEPING = frozenset({"one byte appended", "last segment length raised by one"})
# well-formed files
LEGAL = frozenset({"seg_pixels 65535"})
# refused by the device for what the inspector cannot know (it has no prior)
INSPECTOR_ACCEPTS = LEGAL | {"a foreign prior_id"}
# the sizes still add up, so the inspector and parse_file accept it: only decoding finds the damage
DECODE_ONLY = frozenset({"first segment length +1, second -1"})

TABLE = (TAB, TAB | SEG)        # bit 2 must be set, bit 0 may be
WITHIN = (0, TAB | SEG)         # non-zero, within bits 0 and 2
ONLY_HEADER = (HDR, HDR)
ONLY_SEGMENT = (SEG, SEG)
CLEAN = (0, 0)


def layout(ver, data):
    """Of a well-formed file: tables [(channel, offset)] of the stored tables, segtab, seg_pixels,
    nseg, lens, payload."""
    hdr = HEADER[ver]
    at, tables = hdr, []
    for c in range(R.CH):
        if ver == 1 or (data[28 + (c >> 3)] >> (c & 7)) & 1:
            tables.append((c, at))
            at += 1 + 3 * (data[at] + 1)
    sp, h8, w8 = struct.unpack("<HII", data[6:16])
    nseg = -(-h8 * w8 // sp)
    lens = list(struct.unpack(f"<{nseg}I", data[at:at + 4 * nseg]))
    return dict(tables=tables, segtab=at, seg_pixels=sp, nseg=nseg, lens=lens, payload=at + 4 * nseg)


def _entries(data, off):
    return [struct.unpack("<BH", data[off + 1 + 3 * e:off + 4 + 3 * e]) for e in range(data[off] + 1)]


def _table(entries):
    return bytes([len(entries) - 1]) + b"".join(struct.pack("<BH", s, f) for s, f in entries)


def corruptions(ver, data, rewrite=None):
    """data: a well-formed file of version ver with a stored table of at least two entries and, for
    versions 2 and 3, at least one prior channel.  rewrite(seg_pixels) -> the same latent's file
    under other segments (for the legal case "seg_pixels 65535"; None: left out)."""
    data = bytes(data)
    hdr, lay = HEADER[ver], layout(ver, data)
    segtab, nseg, lens, payload = lay["segtab"], lay["nseg"], lay["lens"], lay["payload"]
    out = {}

    def put(name, d, expected, size=None):
        assert name not in out, name
        out[name] = (bytes(d), len(d) if size is None else size, expected)

    def patch(at, new):
        return data[:at] + bytes(new) + data[at + len(new):]

    # ---- header -----------------------------------------------------------------------------
    put("bad magic", b"NICX" + data[4:], ONLY_HEADER)
    for v in (1, 2, 3, 4):
        if v != ver:
            put(f"version {v}", patch(4, [v]), ONLY_HEADER)
    put("probability bits 11", patch(5, [11]), ONLY_HEADER)
    put("seg_pixels 0", patch(6, [0, 0]), ONLY_HEADER)
    put("h8 0", patch(8, struct.pack("<I", 0)), ONLY_HEADER)
    put("shorter than the header", data[:hdr - 7], ONLY_HEADER)
    if rewrite is not None:
        put("seg_pixels 65535", rewrite(65535), CLEAN)
    if ver != 1:
        h8, = struct.unpack("<I", data[8:12])
        put("H one row too many for h8", patch(16, struct.pack("<I", 8 * h8 + 1)), ONLY_HEADER)
        put("H too small for h8", patch(16, struct.pack("<I", 8 * h8 - 8)), ONLY_HEADER)
        put("W 0", patch(20, struct.pack("<I", 0)), ONLY_HEADER)
        pid, = struct.unpack("<I", data[24:28])
        put("a foreign prior_id", patch(24, struct.pack("<I", pid ^ 0x01000000)), (PRIOR, PRIOR))

    # ---- bookkeeping: the inspector's check alone ----------------------------------------------
    put("one byte appended", data + b"\x00", CLEAN)
    put("last segment length raised by one", patch(segtab + 4 * (nseg - 1), struct.pack("<I", lens[-1] + 1)), CLEAN)

    # ---- truncation: a smaller size, the original bytes still behind it ------------------------
    put("header only", data[:hdr], WITHIN)
    put("truncated by one byte", data[:-1], WITHIN)
    for size in (0, -1, hdr - 1):
        put(f"size {size}", data, ONLY_HEADER, size)
    first = lay["tables"][0][1]  # == hdr: the first stored table's n-1 byte
    cuts = {hdr: "the header's end", hdr + 1: "behind the first table's n-1 byte", first + 3: "inside an entry",
            segtab - 1: "one byte short of the last table's end", segtab: "the last table's end",
            segtab + 1: "one byte into the segment table", segtab + 4 * (nseg // 2) + 2: "inside the segment table",
            payload - 1: "one byte short of the payload", payload: "the segment table's end",
            payload + 1: "the first byte of the payload", len(data) - 1: "one byte before the end"}
    for size, what in sorted(cuts.items()):
        put(f"cut at {what} ({size} of {len(data)})", data, WITHIN, size)

    # ---- tables: a stored table of at least two entries ----------------------------------------
    c, off = next((c, o) for c, o in lay["tables"] if data[o] >= 1)
    ent = _entries(data, off)
    (s0, f0), (s1, f1) = ent[0], ent[1]
    end = off + 1 + 3 * len(ent)

    def retable(entries):
        return data[:off] + _table(entries) + data[end:]

    low = [(s0, f0 - 1), (s1, f1)] if f0 > 1 else [(s0, f0), (s1, f1 - 1)]
    put("freqs sum to 4095", retable(low + ent[2:]), TABLE)
    put("descending symbols", retable([(s1, f0), (s0, f1)] + ent[2:]), TABLE)
    put("equal symbols", retable([(s0, f0), (s0, f1)] + ent[2:]), TABLE)
    put("a freq of 0, the others still summing to 4096", retable([(s0, 0), (s1, f0 + f1)] + ent[2:]), TABLE)
    put("one entry of freq 4097", retable([(s0, 4097)]), TABLE)
    put("two entries of 3000 and 3000", retable([(s0, 3000), (s1, 3000)]), TABLE)
    put("freqs sum to 4097", retable([(s0, f0 + 1)] + ent[1:]), TABLE)
    put("n-1 raised by one", patch(off, [data[off] + 1]), TABLE)
    put("n-1 lowered by one", patch(off, [data[off] - 1]), TABLE)
    # n-1 = 255 on the last stored table of a file that ends inside those 769 bytes: the file is cut
    # there if it is longer
    last = lay["tables"][-1][1]
    put("n-1 255 on the last table, the file ends inside it", patch(last, [255]), TABLE, min(len(data), last + 1 + 3 * 128 + 1))

    # ---- mask (versions 2 and 3) ---------------------------------------------------------------
    if ver != 1:
        stored = {ch for ch, _ in lay["tables"]}
        free = next(i for i in range(R.CH) if i not in stored)
        m = bytearray(data)
        m[28 + (free >> 3)] |= 1 << (free & 7)
        put("a mask bit set with no table behind it", m, WITHIN)
        m = bytearray(data)
        m[28 + (c >> 3)] &= ~(1 << (c & 7)) & 255
        put("a mask bit cleared in front of its table", m, WITHIN)
        put("all twelve mask bytes 0xFF", patch(28, b"\xff" * 12), WITHIN)

    # ---- segment table ---------------------------------------------------------------------------
    def seglen(k, v):
        return patch(segtab + 4 * k, struct.pack("<I", v))

    put("segment length raised by one", seglen(0, lens[0] + 1), ONLY_SEGMENT)
    put("a segment length of 0", seglen(0, 0), ONLY_SEGMENT)
    put("a segment length of 0xFFFFFFFF", seglen(0, 0xFFFFFFFF), ONLY_SEGMENT)
    put("every segment length 0xFFFFFFFF", patch(segtab, b"\xff" * (4 * nseg)), ONLY_SEGMENT)
    if nseg >= 3:  # damage that stays inside segments 0 and 1: every later segment keeps its place
        put("first segment length +1, second -1", patch(segtab, struct.pack("<II", lens[0] + 1, lens[1] - 1)), ONLY_SEGMENT)
    for k in (255, 256):  # the last lane of the offsets' first 256-wide pass, and the first of the second
        if nseg > k + 1:
            put(f"length of segment {k} raised by one", seglen(k, lens[k] + 1), ONLY_SEGMENT)
    return out


def inspector_refuses(name):
    """The inspector's contract applies to the case: NIC_ECORRUPT, and the reference parse_file raises."""
    return name not in INSPECTOR_ACCEPTS | DECODE_ONLY


def as_file(d, size):
    """The file a host reader sees: the slot's first `size` bytes."""
    return d[:max(size, 0)]


def within(status, name, expected):
    """status satisfies the case's masks."""
    must, may = expected
    return status & must == must and status & ~may == 0 and (status != 0 or name in BOOKKEEPING | LEGAL)


# ---- the small bases of the model and the device tests -----------------------------------------
# Version 1: the odd37x53 golden latent (5 x 7) at seg_pixels 3 and 32, and a 17 x 16 latent at
# seg_pixels 1 (272 segments) for the segment-table cases.  Versions 2 and 3: a crafted 9 x 11 latent
# with two own-table channels (0: four symbols the prior gives freq 1; 1: constant, against a uniform
# prior row) and the rest under the prior fitted on the latent itself.

def crafted_9x11():
    rng = np.random.default_rng(41)
    z = np.minimum(rng.geometric(0.3, (99, 96)) - 1, 255).astype(np.uint8)
    z[:, 0] = 10 + np.arange(99) % 4
    z[:, 1] = 255
    return z.reshape(9, 11, 96)


def latent_17x16():
    rng = np.random.default_rng(43)
    return np.minimum(rng.geometric(0.3, (17, 16, 96)) - 1, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def priors_9x11():
    """(static prior, context prior) for the crafted latent."""
    z = crafted_9x11()
    p = R2.fit_prior([z])
    p[0] = [4096 - 255] + [1] * 255
    p[1] = [16] * 256
    anchors, freqs = R3.fit_context_prior([z], p)
    freqs[0] = [list(p[0]) for _ in range(3)]
    freqs[1] = [list(p[1]) for _ in range(3)]
    return p, (anchors, freqs)


@functools.lru_cache(maxsize=None)
def bases():
    """key -> dict(ver, h8, w8, latent, prior, data, cases): cases is corruptions() of data, for the
    17 x 16 base only its segment-table cases."""
    from tests.conftest import load_case

    odd = load_case("odd37x53")["latent"][0]
    p2, p3 = priors_9x11()
    z9, z17 = crafted_9x11(), latent_17x16()
    out = {}

    def add(key, ver, z, prior, write, keep=None):
        data = write(32 if isinstance(key, str) else key[1])
        cases = corruptions(ver, data, write)
        if keep is not None:
            cases = {k: v for k, v in cases.items() if keep(k)}
        out[key] = dict(ver=ver, h8=z.shape[0], w8=z.shape[1], latent=z, prior=prior, data=data, cases=cases)

    add(("v1 5x7", 3), 1, odd, None, lambda sp: R.write_file(odd, sp))
    add(("v1 5x7", 32), 1, odd, None, lambda sp: R.write_file(odd, sp))
    add(("v1 17x16", 1), 1, z17, None, lambda sp: R.write_file(z17, sp), lambda k: "segment" in k and k not in BOOKKEEPING)
    for sp in (3, 32):
        add(("v2 9x11", sp), 2, z9, p2, lambda sp: R2.write_file(z9, p2, sp, (70, 83)))
        add(("v3 9x11", sp), 3, z9, p3, lambda sp: R3.write_file(z9, p3, sp, (70, 83)))
    return out


@functools.lru_cache(maxsize=None)
def model_of(key):
    """name -> (status, latent or None) of the lenient reader model for every case of a base."""
    from tests import rans_read_model as RM

    b = bases()[key]
    return {name: RM.read(b["ver"], d, size, b["h8"], b["w8"], b["prior"]) for name, (d, size, _) in b["cases"].items()}
