"""A small PNG reader for the tests of the device PNG writer: chunk framing with every CRC
checked, the IHDR fields, the inflated IDAT stream (zlib checks the Adler-32), and a walk over the
deflate blocks that counts them by type.  Pure Python, no project code."""
import struct
import zlib
from typing import List, NamedTuple, Tuple

SIGNATURE = bytes([137, 80, 78, 71, 13, 10, 26, 10])


class Png(NamedTuple):
    width: int
    height: int
    bit_depth: int
    colour_type: int
    interlace: int
    chunks: List[Tuple[bytes, int]]  # (type, data length) in file order
    idat: bytes                      # the concatenated IDAT data: one zlib stream
    filtered: bytes                  # its inflated bytes: per row the filter byte and the filtered row

    @property
    def channels(self) -> int:
        return {0: 1, 2: 3, 4: 2, 6: 4, 3: 1}[self.colour_type]

    def filter_bytes(self) -> bytes:
        row = self.width * self.channels * self.bit_depth // 8 + 1
        return self.filtered[::row]


def parse(data: bytes) -> Png:
    """Split a PNG file into chunks; AssertionError on bad framing, a wrong CRC, bytes after IEND
    or a filtered stream of the wrong length (zlib.error on a bad deflate stream or Adler-32)."""
    assert data[:8] == SIGNATURE, "bad signature"
    at, chunks, idat, ihdr = 8, [], b"", None
    while True:
        assert at + 12 <= len(data), "truncated chunk"
        (n,) = struct.unpack(">I", data[at:at + 4])
        typ, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert at + 12 + n <= len(data), "truncated chunk data"
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(typ + body), f"bad CRC in {typ!r}"
        chunks.append((typ, n))
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        at += 12 + n
        if typ == b"IEND":
            break
    assert at == len(data), "bytes after IEND"
    assert chunks[0][0] == b"IHDR" and ihdr is not None and ihdr[4] == 0 and ihdr[5] == 0
    png = Png(ihdr[0], ihdr[1], ihdr[2], ihdr[3], ihdr[6], chunks, idat, zlib.decompress(idat))
    assert len(png.filtered) == png.height * (png.width * png.channels * png.bit_depth // 8 + 1)
    return png


class _Bits:
    def __init__(self, data: bytes, byte: int):
        self.d, self.pos = data, 8 * byte

    def peek(self, n: int) -> int:
        i = self.pos >> 3
        return (int.from_bytes(self.d[i:i + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n: int) -> int:
        v = self.peek(n)
        self.pos += n
        return v


def _table(lengths):
    """peeked bits (LSB first) -> (symbol, length) of a canonical code; {} for no codes."""
    maxlen = max(lengths, default=0)
    if maxlen == 0:
        return {}, 0
    code, tab = 0, {}
    for ln in range(1, maxlen + 1):
        for s, l in enumerate(lengths):
            if l == ln:
                rev = int(format(code, f"0{ln}b")[::-1], 2)
                for hi in range(1 << (maxlen - ln)):
                    tab[rev | (hi << ln)] = (s, ln)
                code += 1
        code <<= 1
    return tab, maxlen


def _sym(bits: _Bits, tab, maxlen) -> int:
    s, l = tab[bits.peek(maxlen)]
    bits.pos += l
    return s


_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def deflate_blocks(zdata: bytes) -> List[dict]:
    """Walk the deflate blocks of a zlib stream: a list of {"type": "stored" | "fixed" | "dynamic",
    "final", "symbols" (literals + matches; stored: bytes), "max_len" (longest literal/length code;
    dynamic only), "start_bit"}.  The data is not reconstructed."""
    bits, out = _Bits(zdata, 2), []
    while True:
        start = bits.pos
        final, typ = bits.take(1), bits.take(2)
        assert typ != 3, "reserved block type"
        if typ == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            assert n ^ nn == 0xFFFF, "stored block: LEN / NLEN mismatch"
            bits.pos += 8 * n
            out.append({"type": "stored", "final": final, "symbols": n, "start_bit": start})
        else:
            if typ == 1:
                lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dist = [5] * 30
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[_CL_ORDER[k]] = bits.take(3)
                ctab, cmax = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _sym(bits, ctab, cmax)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.take(3))
                    else:
                        lens += [0] * (11 + bits.take(7))
                assert len(lens) == hlit + hdist
                lit, dist = lens[:hlit], lens[hlit:]
            ltab, lmax = _table(lit)
            dtab, dmax = _table(dist)
            n = 0
            while True:
                s = _sym(bits, ltab, lmax)
                if s == 256:
                    break
                n += 1
                if s > 256:
                    bits.pos += _LEN_EXTRA[s - 257]
                    bits.pos += _DIST_EXTRA[_sym(bits, dtab, dmax)]
            out.append({"type": "fixed" if typ == 1 else "dynamic", "final": final, "symbols": n, "max_len": max(lit),
                        "start_bit": start})
        if final:
            break
    assert (bits.pos + 7) // 8 + 4 == len(zdata), "bytes between the last block and the Adler-32"
    return out
