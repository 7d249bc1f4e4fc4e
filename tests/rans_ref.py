"""Pure-Python writer and reader of the .nic container (version 1), restated from the format
text in DESIGN.md ("The .nic container"); the device coder (csrc/nic_rans.hip) is checked
against it.  Nothing here touches the library.

A file: 16-byte header ("NICR", u8 version 1, u8 probability bits 12, u16 seg_pixels, u32 h8,
u32 w8), 96 channel tables (u8 n-1, n x (u8 symbol, u16 freq)), nseg u32 segment lengths, the
segments.  Segment k codes the latent bytes [k K, min((k+1) K, 96 h8 w8)), K = 96 seg_pixels,
in NHWC order; byte j is a symbol of channel j % 96.  Byte-wise rANS, u32 state, L = 2^23.
"""
import math
import struct

import numpy as np

MAGIC = b"NICR"
PROB_BITS = 12
M = 1 << PROB_BITS
L = 1 << 23
CH = 96


def normalise(counts):
    """256 counts -> 256 freqs: max(1, floor(c 4096 / N)) per used symbol; a deficit goes onto
    the largest entry, a surplus is taken one at a time from the currently largest entry (the
    lowest symbol on ties), which never takes an entry below 1."""
    counts = [int(c) for c in counts]
    n = sum(counts)
    f = [max(1, c * M // n) if c else 0 for c in counts]
    diff = M - sum(f)
    if diff > 0:
        f[max(range(256), key=lambda s: (f[s], -s))] += diff
    while diff < 0:
        f[max(range(256), key=lambda s: (f[s], -s))] -= 1
        diff += 1
    assert sum(f) == M and all((c > 0) == (v > 0) for c, v in zip(counts, f))
    return f


def tables_of_latent(z):
    """(h8, w8, 96) u8 -> 96 lists of 256 freqs."""
    flat = np.asarray(z).reshape(-1, CH)
    return [normalise(np.bincount(flat[:, c], minlength=256)) for c in range(CH)]


def _starts(f):
    st, run = [], 0
    for v in f:
        st.append(run)
        run += v
    return st


def encode_segment(symbols, first_channel, freqs, starts):
    """The bytes of one segment: symbols[j] belongs to channel (first_channel + j) % 96."""
    out = bytearray()
    x = L
    for j in range(len(symbols) - 1, -1, -1):
        c = (first_channel + j) % CH
        s = symbols[j]
        fr, st = freqs[c][s], starts[c][s]
        assert fr > 0, "symbol without a table entry"
        x_max = fr << 19
        while x >= x_max:
            out.append(x & 255)
            x >>= 8
        x = ((x // fr) << PROB_BITS) + (x % fr) + st
    for _ in range(4):
        out.append(x & 255)
        x >>= 8
    out.reverse()
    return bytes(out)


def write_file(z, seg_pixels=32, tables=None):
    """(h8, w8, 96) u8 latent -> the file's bytes.  tables: 96 x 256 freqs (default: this
    module's normalisation of the latent's own counts)."""
    z = np.ascontiguousarray(z, dtype=np.uint8)
    h8, w8, ch = z.shape
    assert ch == CH and 1 <= seg_pixels <= 65535
    tables = tables_of_latent(z) if tables is None else tables
    starts = [_starts(f) for f in tables]
    out = bytearray(MAGIC + struct.pack("<BBHII", 1, PROB_BITS, seg_pixels, h8, w8))
    for f in tables:
        used = [s for s in range(256) if f[s]]
        out.append(len(used) - 1)
        for s in used:
            out += struct.pack("<BH", s, f[s])
    flat = z.reshape(-1).tolist()
    k = CH * seg_pixels
    segs = [encode_segment(flat[a:a + k], 0, tables, starts) for a in range(0, len(flat), k)]
    for s in segs:
        out += struct.pack("<I", len(s))
    for s in segs:
        out += s
    return bytes(out)


def parse_file(data):
    """-> dict(h8, w8, seg_pixels, tables (96 x 256 freqs), seg_lengths, payload (offset),
    table_bytes).  Raises ValueError on a malformed file."""
    data = bytes(data)
    if len(data) < 16 or data[:4] != MAGIC:
        raise ValueError("bad magic")
    ver, bits, seg_pixels, h8, w8 = struct.unpack("<BBHII", data[4:16])
    if ver != 1 or bits != PROB_BITS or seg_pixels < 1 or h8 * w8 == 0:
        raise ValueError("bad header")
    at, tables = 16, []
    for c in range(CH):
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
    return dict(h8=h8, w8=w8, seg_pixels=seg_pixels, tables=tables, seg_lengths=lens, payload=at + 4 * nseg,
                table_bytes=at - 16)


def decode_segment(data, count, first_channel, freqs, starts, lut):
    """count symbols from one segment's bytes; ValueError unless it ends with x == L on its last byte."""
    if len(data) < 4:
        raise ValueError("segment shorter than its state")
    x = int.from_bytes(data[:4], "big")
    p, out = 4, []
    for j in range(count):
        c = (first_channel + j) % CH
        slot = x & (M - 1)
        s = lut[c][slot]
        x = freqs[c][s] * (x >> PROB_BITS) + slot - starts[c][s]
        while x < L:
            if p >= len(data):
                raise ValueError("segment ran out of bytes")
            x = (x << 8) | data[p]
            p += 1
        out.append(s)
    if x != L or p != len(data):
        raise ValueError("segment did not end at the initial state on its last byte")
    return out


def read_file(data):
    """The file's bytes -> (h8, w8, 96) u8 latent."""
    info = parse_file(data)
    tables = info["tables"]
    starts = [_starts(f) for f in tables]
    lut = [np.repeat(np.arange(256), f).tolist() for f in tables]
    h8, w8, k = info["h8"], info["w8"], CH * info["seg_pixels"]
    total, at, out = CH * h8 * w8, info["payload"], []
    for i, n in enumerate(info["seg_lengths"]):
        out += decode_segment(data[at:at + n], min(k, total - i * k), 0, tables, starts, lut)
        at += n
    return np.array(out, dtype=np.uint8).reshape(h8, w8, CH)


def ideal_payload_bytes(z, tables):
    """sum count log2(4096 / freq) / 8: the cost of the latent under the stored tables."""
    flat = np.asarray(z).reshape(-1, CH)
    bits = 0.0
    for c in range(CH):
        cnt = np.bincount(flat[:, c], minlength=256)
        for s in np.nonzero(cnt)[0]:
            bits += int(cnt[s]) * math.log2(M / tables[c][s])
    return bits / 8.0
