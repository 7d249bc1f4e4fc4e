"""Pure-Python restatement of the .nic container's version 3 ("The .nic container,
version 3"): the context prior and its fitting, the context of a byte, the per-channel choice,
the file writer and reader, and the .nicc context-prior file.  The coder's arithmetic is
rans_ref's, the cost table and the normalisation rule are rans2_ref's.  Nothing here touches the
library.

A context prior: (anchors, freqs) with 96 anchors (u8) and 96 x 3 rows of 256 freqs, each in
1..4096, every row summing to 4096; its id is the CRC-32 of the anchors followed by the freqs as
little-endian u16 (channel-major, then context, then symbol).  A file is version 2's with version
byte 3.  The byte at segment-relative offset j (channel c = j % 96, pixel q = j // 96) is coded
under row (c, k): k = 0 if q == 0, else min(2, |z[j - 96] - anchor[c]|).  A masked channel is
coded under its own table in every context.
"""
import struct
import zlib

import numpy as np

from tests import rans2_ref as R2
from tests import rans_ref as R

CH, M, L = R.CH, R.M, R.L
CTX = 3
HEADER = 40
CPRIOR_MAGIC = b"NICC"
CPRIOR_BYTES = 16 + CH + CH * CTX * 256 * 2


def anchors_of(static_prior):
    """The argmax of every row of a static prior (96 x 256), the lowest symbol on ties."""
    return [max(range(256), key=lambda s: (int(row[s]), -s)) for row in static_prior]


def contexts_of(z, anchors, seg_pixels):
    """(h8, w8, 96) u8 -> (npix, 96) contexts in 0..2."""
    flat = np.asarray(z).reshape(-1, CH).astype(np.int64)
    d = np.minimum(2, np.abs(flat[:-1] - np.asarray(anchors, np.int64)[None]))
    ctx = np.zeros_like(flat)
    ctx[1:] = d
    ctx[::seg_pixels] = 0
    return ctx


def context_counts(z, anchors, seg_pixels=32):
    """(h8, w8, 96) u8 -> (96, 3, 256) counts."""
    flat = np.asarray(z).reshape(-1, CH).astype(np.int64)
    ctx = contexts_of(z, anchors, seg_pixels)
    out = np.zeros((CH, CTX, 256), np.int64)
    for c in range(CH):
        out[c] = np.bincount(ctx[:, c] * 256 + flat[:, c], minlength=CTX * 256).reshape(CTX, 256)
    return out


def counts_of(latents, anchors, seg_pixels=32):
    """An iterable of (h8, w8, 96) u8 latents -> (96, 3, 256) counts."""
    acc = np.zeros((CH, CTX, 256), np.int64)
    for z in latents:
        acc += context_counts(z, anchors, seg_pixels)
    return acc


def normalise_counts(counts):
    return [[R2.normalise_prior(row) for row in ch] for ch in counts]


def fit_context_prior(latents, static_prior=None, seg_pixels=32):
    """-> (anchors, freqs).  The anchors come from static_prior (default: fitted on the latents)."""
    latents = list(latents)
    if static_prior is None:
        static_prior = R2.fit_prior(latents)
    anchors = anchors_of(static_prior)
    return anchors, normalise_counts(counts_of(latents, anchors, seg_pixels))


def uniform_context_prior():
    return [0] * CH, [[[16] * 256 for _ in range(CTX)] for _ in range(CH)]


def replicate(static_prior, anchors=None):
    """The context prior whose three rows all equal the static prior's row."""
    return (anchors_of(static_prior) if anchors is None else list(anchors),
            [[[int(v) for v in row] for _ in range(CTX)] for row in static_prior])


def prior_bytes(cprior):
    anchors, freqs = cprior
    return bytes(int(a) for a in anchors) + np.asarray(freqs, dtype="<u2").reshape(CH, CTX, 256).tobytes()


def prior_id(cprior):
    return zlib.crc32(prior_bytes(cprior))


def check_prior(cprior):
    anchors, freqs = cprior
    if len(anchors) != CH or any(not 0 <= int(a) <= 255 for a in anchors) or len(freqs) != CH:
        raise ValueError("bad context prior")
    for c, rows in enumerate(freqs):
        if len(rows) != CTX:
            raise ValueError(f"channel {c}: not {CTX} contexts")
        for k, row in enumerate(rows):
            if len(row) != 256 or any(not 1 <= int(v) <= M for v in row) or sum(int(v) for v in row) != M:
                raise ValueError(f"channel {c} context {k}: bad row")


def write_nicc(cprior):
    check_prior(cprior)
    return CPRIOR_MAGIC + struct.pack("<BBHIB3x", 1, R.PROB_BITS, CH, prior_id(cprior), CTX) + prior_bytes(cprior)


def read_nicc(data):
    data = bytes(data)
    if len(data) != CPRIOR_BYTES or data[:4] != CPRIOR_MAGIC:
        raise ValueError("not a .nicc file")
    ver, bits, ch, pid, ctx, z0, z1, z2 = struct.unpack("<BBHIBBBB", data[4:16])
    if (ver, bits, ch, ctx, z0, z1, z2) != (1, R.PROB_BITS, CH, CTX, 0, 0, 0):
        raise ValueError("bad .nicc header")
    anchors = list(data[16:16 + CH])
    freqs = np.frombuffer(data[16 + CH:], "<u2").reshape(CH, CTX, 256).astype(int).tolist()
    check_prior((anchors, freqs))
    if prior_id((anchors, freqs)) != pid:
        raise ValueError("prior_id does not match the anchors and freqs")
    return anchors, freqs


def choose(ctx_counts, prior_rows):
    """(3, 256) counts of one channel, its 3 prior rows -> (keep, own freqs)."""
    total = [sum(int(ctx_counts[k][s]) for k in range(CTX)) for s in range(256)]
    f = R.normalise(total)
    n = sum(1 for v in f if v)
    own = sum(c * R2.COST16[v] for c, v in zip(total, f)) + ((8 * (1 + 3 * n)) << 16)
    pri = sum(int(ctx_counts[k][s]) * R2.COST16[int(prior_rows[k][s])] for k in range(CTX) for s in range(256))
    return own < pri, f


def tables_of_latent(z, cprior, seg_pixels=32):
    """(h8, w8, 96) u8 -> (mask: 96 bools, tables: 96 x 3 x 256 freqs as coded)."""
    anchors, freqs = cprior
    counts = context_counts(z, anchors, seg_pixels)
    mask, tables = [], []
    for c in range(CH):
        keep, f = choose(counts[c], freqs[c])
        mask.append(keep)
        tables.append([f] * CTX if keep else [[int(v) for v in row] for row in freqs[c]])
    return mask, tables


def encode_segment(symbols, ctx, tables, starts):
    """The bytes of one segment that begins at channel 0: symbols[j] of channel j % 96 under row ctx[j]."""
    out = bytearray()
    x = L
    for j in range(len(symbols) - 1, -1, -1):
        c, s, k = j % CH, symbols[j], ctx[j]
        fr, st = tables[c][k][s], starts[c][k][s]
        assert fr > 0, "symbol without a table entry"
        x_max = fr << 19
        while x >= x_max:
            out.append(x & 255)
            x >>= 8
        x = ((x // fr) << R.PROB_BITS) + (x % fr) + st
    for _ in range(4):
        out.append(x & 255)
        x >>= 8
    out.reverse()
    return bytes(out)


def write_file(z, cprior, seg_pixels=32, size=None):
    """(h8, w8, 96) u8 latent of an H x W image (size; default 8 h8 x 8 w8) -> the file's bytes."""
    z = np.ascontiguousarray(z, dtype=np.uint8)
    h8, w8, ch = z.shape
    H, W = size if size is not None else (8 * h8, 8 * w8)
    assert ch == CH and 1 <= seg_pixels <= 65535 and -(-H // 8) == h8 and -(-W // 8) == w8
    mask, tables = tables_of_latent(z, cprior, seg_pixels)
    starts = [[R._starts(f) for f in rows] for rows in tables]
    bits = bytearray(12)
    for c in range(CH):
        if mask[c]:
            bits[c >> 3] |= 1 << (c & 7)
    out = bytearray(R.MAGIC + struct.pack("<BBHIIIII", 3, R.PROB_BITS, seg_pixels, h8, w8, H, W, prior_id(cprior)) + bits)
    assert len(out) == HEADER
    for c in range(CH):
        if mask[c]:
            used = [s for s in range(256) if tables[c][0][s]]
            out.append(len(used) - 1)
            for s in used:
                out += struct.pack("<BH", s, tables[c][0][s])
    flat = z.reshape(-1).tolist()
    ctx = contexts_of(z, cprior[0], seg_pixels).reshape(-1).tolist()
    k = CH * seg_pixels
    segs = [encode_segment(flat[a:a + k], ctx[a:a + k], tables, starts) for a in range(0, len(flat), k)]
    for s in segs:
        out += struct.pack("<I", len(s))
    for s in segs:
        out += s
    return bytes(out)


def parse_file(data, cprior=None):
    """-> dict(h8, w8, seg_pixels, H, W, prior_id, mask, tables (masked channels: the file's table
    three times; the others: the context prior's rows, or None without one), seg_lengths, payload,
    table_bytes).  ValueError on a malformed file or a context prior of another id."""
    data = bytes(data)
    if len(data) < HEADER or data[:4] != R.MAGIC:
        raise ValueError("bad magic")
    ver, bits, seg_pixels, h8, w8, H, W, pid = struct.unpack("<BBHIIIII", data[4:28])
    if ver != 3 or bits != R.PROB_BITS or seg_pixels < 1 or h8 * w8 == 0:
        raise ValueError("bad header")
    if -(-H // 8) != h8 or -(-W // 8) != w8:
        raise ValueError("H x W does not give h8 x w8")
    if cprior is not None and prior_id(cprior) != pid:
        raise ValueError(f"context prior {prior_id(cprior):08x} is not the file's {pid:08x}")
    mask = [bool((data[28 + (c >> 3)] >> (c & 7)) & 1) for c in range(CH)]
    at, tables = HEADER, []
    for c in range(CH):
        if not mask[c]:
            tables.append(None if cprior is None else [[int(v) for v in row] for row in cprior[1][c]])
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
        tables.append([f] * CTX)
        at += 1 + 3 * n
    nseg = -(-h8 * w8 // seg_pixels)
    if at + 4 * nseg > len(data):
        raise ValueError("segment table truncated")
    lens = list(struct.unpack(f"<{nseg}I", data[at:at + 4 * nseg]))
    if at + 4 * nseg + sum(lens) != len(data):
        raise ValueError("sizes do not add up")
    return dict(h8=h8, w8=w8, seg_pixels=seg_pixels, H=H, W=W, prior_id=pid, mask=mask, tables=tables, seg_lengths=lens,
                payload=at + 4 * nseg, table_bytes=at - HEADER)


def decode_segment(data, count, anchors, tables, starts, lut):
    """count symbols of a segment that begins at channel 0; ValueError unless it ends with x == L on
    its last byte."""
    if len(data) < 4:
        raise ValueError("segment shorter than its state")
    x = int.from_bytes(data[:4], "big")
    p, out = 4, []
    for j in range(count):
        c = j % CH
        k = 0 if j < CH else min(2, abs(out[j - CH] - anchors[c]))
        slot = x & (M - 1)
        s = lut[c][k][slot]
        x = tables[c][k][s] * (x >> R.PROB_BITS) + slot - starts[c][k][s]
        while x < L:
            if p >= len(data):
                raise ValueError("segment ran out of bytes")
            x = (x << 8) | data[p]
            p += 1
        out.append(s)
    if x != L or p != len(data):
        raise ValueError("segment did not end at the initial state on its last byte")
    return out


def read_file(data, cprior):
    """The file's bytes -> (h8, w8, 96) u8 latent."""
    info = parse_file(data, cprior)
    tables = info["tables"]
    starts = [[R._starts(f) for f in rows] for rows in tables]
    lut = [[np.repeat(np.arange(256), f).tolist() for f in rows] for rows in tables]
    h8, w8, k = info["h8"], info["w8"], CH * info["seg_pixels"]
    total, at, out = CH * h8 * w8, info["payload"], []
    for i, n in enumerate(info["seg_lengths"]):
        out += decode_segment(data[at:at + n], min(k, total - i * k), cprior[0], tables, starts, lut)
        at += n
    return np.array(out, dtype=np.uint8).reshape(h8, w8, CH)
