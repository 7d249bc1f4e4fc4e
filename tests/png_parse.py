"""A small PNG reader for the tests of the device PNG writer and reader: chunk framing with every
CRC checked, the IHDR fields, the inflated IDAT stream (zlib checks the Adler-32), and a walk over the
deflate blocks that reports, per block, what a test needs to prove that a stream reaches the edge it
was built for: the code lengths declared and used, the distances, the header's own symbols, where the
block starts in the input and in the output.  Pure Python, no project code."""
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

    def peek(self, n: int) -> int:  # n <= 25
        i = self.pos >> 3
        return (int.from_bytes(self.d[i:i + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n: int) -> int:
        v = self.peek(n)
        self.pos += n
        return v


def _table(lengths):
    """peeked bits (LSB first) -> (symbol, length) of a canonical code, and its longest length.  The
    code need not be complete: bits that are no code have no entry.  {} for no codes."""
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


def _sym(bits: _Bits, tab, maxlen):
    """(symbol, its code's length); AssertionError where the bits are no code of the set."""
    e = tab.get(bits.peek(maxlen)) if maxlen else None
    assert e is not None, "bits that are no code of the set"
    bits.pos += e[1]
    return e


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def deflate_blocks(zdata: bytes, trailing: bool = False) -> List[dict]:
    """Walk the deflate blocks of a zlib stream.  Per block:
      "type"        "stored" | "fixed" | "dynamic"
      "final"       BFINAL
      "symbols"     literals + matches (stored: bytes)
      "start_bit"   where its header starts in zdata; "data_byte" (stored): where its bytes start
      "out_start"   how many bytes the blocks before it produced
    and for the Huffman blocks
      "max_len", "dist_max_len"    the longest literal/length and distance code the block declares
      "used_lens", "dist_used_lens"  the set of code lengths it really decodes (literal/length: the
                                   end-of-block code included)
      "used_len", "dist_used_len"  the longest of those (0: none)
      "max_dist"    the largest distance (0: no match)
      "matches"     its number of matches; "len_symbols": the set of length symbols they use
      "reach"       the most bytes a match goes back beyond the block's own first byte (<= 0: none does)
      "far"         [(output offset, length, distance)] of the matches with distance >= 16384
    and for the dynamic ones
      "hlit", "hdist", "hclen", "cl_lens" (the 19 code-length code lengths),
      "cl_symbols"  [(symbol, repeat, index of the first length it writes)], "lit_lens", "dist_lens".
    Neither set has to be complete.  The data is not reconstructed.  trailing: bytes may follow the
    Adler-32 (zlib.decompress ignores them); otherwise the stream must end with it."""
    bits, out, produced = _Bits(zdata, 2), [], 0
    while True:
        start = bits.pos
        final, typ = bits.take(1), bits.take(2)
        assert typ != 3, "reserved block type"
        blk = {"final": final, "start_bit": start, "out_start": produced}
        if typ == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            assert n ^ nn == 0xFFFF, "stored block: LEN / NLEN mismatch"
            blk.update(type="stored", symbols=n, data_byte=bits.pos >> 3)
            bits.pos += 8 * n
            assert bits.pos <= 8 * len(zdata), "stored block runs past the input"
            produced += n
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
                lens, cls = [], []
                while len(lens) < hlit + hdist:
                    s, _ = _sym(bits, ctab, cmax)
                    at = len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.take(3))
                    else:
                        lens += [0] * (11 + bits.take(7))
                    cls.append((s, len(lens) - at, at))
                assert len(lens) == hlit + hdist
                lit, dist = lens[:hlit], lens[hlit:]
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl, cl_symbols=cls, lit_lens=lit, dist_lens=dist)
            ltab, lmax = _table(lit)
            dtab, dmax = _table(dist)
            n, matches, used, dused, lsyms, max_dist, reach, far = 0, 0, set(), set(), set(), 0, -(1 << 40), []
            block_start = produced
            while True:
                s, ln = _sym(bits, ltab, lmax)
                used.add(ln)
                if s == 256:
                    break
                n += 1
                if s < 256:
                    produced += 1
                    continue
                assert s <= 285, "length symbol 286 or 287"
                length = _LEN_BASE[s - 257] + bits.take(_LEN_EXTRA[s - 257])
                d, dl = _sym(bits, dtab, dmax)
                assert d <= 29, "distance symbol 30 or 31"
                distance = _DIST_BASE[d] + bits.take(_DIST_EXTRA[d])
                assert distance <= produced, "distance beyond the bytes produced"
                dused.add(dl)
                lsyms.add(s)
                matches += 1
                max_dist = max(max_dist, distance)
                reach = max(reach, distance - (produced - block_start))
                if distance >= 16384:
                    far.append((produced, length, distance))
                produced += length
            assert bits.pos <= 8 * len(zdata), "the block runs past the input"
            blk.update(type="fixed" if typ == 1 else "dynamic", symbols=n, max_len=max(lit), dist_max_len=max(dist, default=0),
                       used_lens=used, dist_used_lens=dused, used_len=max(used), dist_used_len=max(dused, default=0),
                       max_dist=max_dist, matches=matches, len_symbols=lsyms, reach=reach if matches else 0, far=far)
        out.append(blk)
        if final:
            break
    end = (bits.pos + 7) // 8 + 4
    assert end <= len(zdata), "the stream ends before its Adler-32"
    assert trailing or end == len(zdata), "bytes between the last block and the Adler-32"
    return out
