"""PNG files built by hand for the tests of the device PNG reader: a chosen filter per row, chosen
zlib settings, a chosen IDAT chunk size, optional ancillary chunks; and framing for a hand-written
deflate stream, with an Adler-32 that is right or deliberately wrong.  Pure Python + NumPy, no
project code."""
import struct
import zlib

import numpy as np

SIGNATURE = bytes([137, 80, 78, 71, 13, 10, 26, 10])


def chunk(typ: bytes, body: bytes = b"") -> bytes:
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(img: np.ndarray, filters) -> bytes:
    """The filtered stream of img (H, W) or (H, W, C) u8: filters is one PNG filter (0..4) for every
    row or a sequence with one per row."""
    a = np.ascontiguousarray(img, np.uint8)
    h = a.shape[0]
    bpp = 1 if a.ndim == 2 else a.shape[2]
    rows = a.reshape(h, -1).astype(np.int32)
    wb = rows.shape[1]
    fs = [filters] * h if isinstance(filters, int) else list(filters)
    assert len(fs) == h
    out = bytearray()
    zero = np.zeros(wb, np.int32)
    for r in range(h):
        x, up = rows[r], rows[r - 1] if r else zero
        left = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if wb > bpp else np.zeros(wb, np.int32)
        upleft = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if wb > bpp else np.zeros(wb, np.int32)
        f = fs[r]
        if f == 0:
            pred = zero
        elif f == 1:
            pred = left
        elif f == 2:
            pred = up
        elif f == 3:
            pred = (left + up) >> 1
        elif f == 4:
            pred = np.array([_paeth(int(p), int(q), int(s)) for p, q, s in zip(left, up, upleft)], np.int32)
        else:  # not a PNG filter: the bytes go in as they are (for the reader's status test)
            pred = zero
        out.append(f)
        out += ((x - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, wbits: int = 15, mem_level: int = 8) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem_level, strategy)
    return c.compress(data) + c.flush()


def ihdr(h: int, w: int, colour: int, depth: int = 8, interlace: int = 0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))


def frame(h: int, w: int, channels: int, zstream: bytes, idat_size: int = 65536, before=(), between=(), after=()) -> bytes:
    """A PNG file around a finished zlib stream, cut into IDATs of idat_size bytes.  before / after:
    (type, body) chunks between IHDR and the first IDAT / between the last IDAT and IEND; between:
    chunks put after the first IDAT (which breaks the file when there is a second IDAT)."""
    colour = {1: 0, 3: 2, 2: 4, 4: 6}[channels]
    out = [SIGNATURE, ihdr(h, w, colour)]
    out += [chunk(t, b) for t, b in before]
    parts = [zstream[i:i + idat_size] for i in range(0, len(zstream), idat_size)] or [b""]
    for k, p in enumerate(parts):
        out.append(chunk(b"IDAT", p))
        if k == 0:
            out += [chunk(t, b) for t, b in between]
    out += [chunk(t, b) for t, b in after]
    out.append(chunk(b"IEND"))
    return b"".join(out)


def make_png(img: np.ndarray, filters=0, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, wbits: int = 15,
             idat_size: int = 65536, **chunks) -> bytes:
    a = np.asarray(img, np.uint8)
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    return frame(h, w, ch, deflate(filter_rows(a, filters), level, strategy, wbits), idat_size, **chunks)


def zlib_wrap(raw_deflate: bytes, data: bytes, adler_delta: int = 0) -> bytes:
    """78 01 | a hand-written deflate stream | the Adler-32 of data (plus adler_delta)."""
    return b"\x78\x01" + raw_deflate + struct.pack(">I", (zlib.adler32(data) + adler_delta) & 0xFFFFFFFF)


class BitWriter:
    """Deflate's bit order: values LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.bits = []

    def put(self, value: int, n: int):
        self.bits += [(value >> i) & 1 for i in range(n)]
        return self

    def code(self, code: int, n: int):
        self.bits += [(code >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def fixed_literal(self, v: int):
        return self.code(0x30 + v, 8) if v < 144 else self.code(0x190 + v - 144, 9)

    def bytes(self) -> bytes:
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))
