"""Pure-Python restatement of the .nic container's version 2 ("The .nic container,
version 2"): the prior and its normalisation, the cost table, the per-channel choice, the file
writer and reader, and the .nicp prior file.  The coder itself is rans_ref's.  Nothing here
touches the library.

A prior: 96 rows of 256 freqs, each in 1..4096, every row summing to 4096; its id is the CRC-32
of the freqs as little-endian u16, channel-major.  A file: 40-byte header ("NICR", u8 version 2,
u8 probability bits 12, u16 seg_pixels, u32 h8, u32 w8, u32 H, u32 W, u32 prior_id, 12-byte
channel mask), a version-1 table for every masked channel, then version 1's segment table and
segments.
"""
import math
import struct
import zlib

import numpy as np

from tests import rans_ref as R

CH, M = R.CH, R.M
HEADER = 40
PRIOR_MAGIC = b"NICP"
PRIOR_BYTES = 16 + CH * 256 * 2

COST16 = [0] + [int(math.floor((12 - math.log2(f)) * 65536 + 0.5)) for f in range(1, M + 1)]


def normalise_prior(counts):
    """256 accumulated counts -> 256 freqs, all >= 1: version 1's rule with every symbol "used"."""
    counts = [int(c) for c in counts]
    n = sum(counts)
    if n == 0:
        return [16] * 256
    f = [max(1, c * M // n) for c in counts]
    diff = M - sum(f)
    if diff > 0:
        f[max(range(256), key=lambda s: (f[s], -s))] += diff
    while diff < 0:
        f[max(range(256), key=lambda s: (f[s], -s))] -= 1
        diff += 1
    assert sum(f) == M and min(f) >= 1
    return f


def counts_of(latents):
    """An iterable of (..., 96) u8 latents -> (96, 256) counts."""
    acc = np.zeros((CH, 256), np.int64)
    for z in latents:
        flat = np.asarray(z).reshape(-1, CH)
        for c in range(CH):
            acc[c] += np.bincount(flat[:, c], minlength=256)
    return acc


def fit_prior(latents):
    return [normalise_prior(row) for row in counts_of(latents)]


def uniform_prior():
    return [[16] * 256 for _ in range(CH)]


def prior_bytes(prior):
    return np.asarray(prior, dtype="<u2").reshape(CH, 256).tobytes()


def prior_id(prior):
    return zlib.crc32(prior_bytes(prior))


def check_prior(prior):
    for c, row in enumerate(prior):
        if len(row) != 256 or any(not 1 <= int(v) <= M for v in row) or sum(int(v) for v in row) != M:
            raise ValueError(f"channel {c}: bad prior row")


def write_nicp(prior):
    check_prior(prior)
    return PRIOR_MAGIC + struct.pack("<BBHII", 1, R.PROB_BITS, CH, prior_id(prior), 0) + prior_bytes(prior)


def read_nicp(data):
    data = bytes(data)
    if len(data) != PRIOR_BYTES or data[:4] != PRIOR_MAGIC:
        raise ValueError("not a .nicp file")
    ver, bits, ch, pid, zero = struct.unpack("<BBHII", data[4:16])
    if (ver, bits, ch, zero) != (1, R.PROB_BITS, CH, 0):
        raise ValueError("bad .nicp header")
    prior = np.frombuffer(data[16:], "<u2").reshape(CH, 256).astype(int).tolist()
    check_prior(prior)
    if prior_id(prior) != pid:
        raise ValueError("prior_id does not match the freqs")
    return prior


def choose(counts, prior_row):
    """-> (keep, own freqs): the channel keeps its own table iff it is strictly cheaper."""
    counts = [int(c) for c in counts]
    f = R.normalise(counts)
    n = sum(1 for v in f if v)
    own = sum(c * COST16[v] for c, v in zip(counts, f)) + ((8 * (1 + 3 * n)) << 16)
    pri = sum(c * COST16[v] for c, v in zip(counts, prior_row))
    return own < pri, f


def tables_of_latent(z, prior):
    """(h8, w8, 96) u8 -> (mask: 96 bools, tables: 96 x 256 freqs as coded)."""
    flat = np.asarray(z).reshape(-1, CH)
    mask, tables = [], []
    for c in range(CH):
        keep, f = choose(np.bincount(flat[:, c], minlength=256), prior[c])
        mask.append(keep)
        tables.append(f if keep else [int(v) for v in prior[c]])
    return mask, tables


def write_file(z, prior, seg_pixels=32, size=None):
    """(h8, w8, 96) u8 latent of an H x W image (size; default 8 h8 x 8 w8) -> the file's bytes."""
    z = np.ascontiguousarray(z, dtype=np.uint8)
    h8, w8, ch = z.shape
    H, W = size if size is not None else (8 * h8, 8 * w8)
    assert ch == CH and 1 <= seg_pixels <= 65535 and -(-H // 8) == h8 and -(-W // 8) == w8
    mask, tables = tables_of_latent(z, prior)
    starts = [R._starts(f) for f in tables]
    bits = bytearray(12)
    for c in range(CH):
        if mask[c]:
            bits[c >> 3] |= 1 << (c & 7)
    out = bytearray(R.MAGIC + struct.pack("<BBHIIIII", 2, R.PROB_BITS, seg_pixels, h8, w8, H, W, prior_id(prior)) + bits)
    assert len(out) == HEADER
    for c in range(CH):
        if mask[c]:
            used = [s for s in range(256) if tables[c][s]]
            out.append(len(used) - 1)
            for s in used:
                out += struct.pack("<BH", s, tables[c][s])
    flat = z.reshape(-1).tolist()
    k = CH * seg_pixels
    segs = [R.encode_segment(flat[a:a + k], 0, tables, starts) for a in range(0, len(flat), k)]
    for s in segs:
        out += struct.pack("<I", len(s))
    for s in segs:
        out += s
    return bytes(out)


def parse_file(data, prior=None):
    """-> dict(h8, w8, seg_pixels, H, W, prior_id, mask, tables (masked channels: the file's; the
    others: the prior's row, or None without a prior), seg_lengths, payload, table_bytes).
    ValueError on a malformed file or a prior of another id."""
    data = bytes(data)
    if len(data) < HEADER or data[:4] != R.MAGIC:
        raise ValueError("bad magic")
    ver, bits, seg_pixels, h8, w8, H, W, pid = struct.unpack("<BBHIIIII", data[4:28])
    if ver != 2 or bits != R.PROB_BITS or seg_pixels < 1 or h8 * w8 == 0:
        raise ValueError("bad header")
    if -(-H // 8) != h8 or -(-W // 8) != w8:
        raise ValueError("H x W does not give h8 x w8")
    if prior is not None and prior_id(prior) != pid:
        raise ValueError(f"prior {prior_id(prior):08x} is not the file's {pid:08x}")
    mask = [bool((data[28 + (c >> 3)] >> (c & 7)) & 1) for c in range(CH)]
    at, tables = HEADER, []
    for c in range(CH):
        if not mask[c]:
            tables.append(None if prior is None else [int(v) for v in prior[c]])
            continue
        if at >= len(data) or at + 1 + 3 * (data[at] + 1) > len(data):
            raise ValueError(f"channel {c}: table truncated")
        n = data[at] + 1
        f, prev = [0] * 256, -1
        for e in range(n):
            s, fr = struct.unpack("<BH", data[at + 1 + 3 * e:at + 4 + 3 * e])
            if s <= prev or not 1 <= fr <= M:
                raise ValueError(f"channel {c}: bad table entry")
            f[s], prev = fr, s
        if sum(f) != M:
            raise ValueError(f"channel {c}: freqs sum to {sum(f)}")
        tables.append(f)
        at += 1 + 3 * n
    nseg = -(-h8 * w8 // seg_pixels)
    if at + 4 * nseg > len(data):
        raise ValueError("segment table truncated")
    lens = list(struct.unpack(f"<{nseg}I", data[at:at + 4 * nseg]))
    if at + 4 * nseg + sum(lens) != len(data):
        raise ValueError("sizes do not add up")
    return dict(h8=h8, w8=w8, seg_pixels=seg_pixels, H=H, W=W, prior_id=pid, mask=mask, tables=tables, seg_lengths=lens,
                payload=at + 4 * nseg, table_bytes=at - HEADER)


def read_file(data, prior):
    """The file's bytes -> (h8, w8, 96) u8 latent."""
    info = parse_file(data, prior)
    tables = info["tables"]
    starts = [R._starts(f) for f in tables]
    lut = [np.repeat(np.arange(256), f).tolist() for f in tables]
    h8, w8, k = info["h8"], info["w8"], CH * info["seg_pixels"]
    total, at, out = CH * h8 * w8, info["payload"], []
    for i, n in enumerate(info["seg_lengths"]):
        out += R.decode_segment(data[at:at + n], min(k, total - i * k), 0, tables, starts, lut)
        at += n
    return np.array(out, dtype=np.uint8).reshape(h8, w8, CH)
