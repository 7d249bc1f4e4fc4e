"""PNG files built by hand for the tests of the device PNG reader: a chosen filter per row, chosen
zlib settings, a chosen IDAT chunk size, optional ancillary chunks; a deflate writer (Deflate: stored,
fixed and dynamic blocks in one bit stream, code lengths and code-length symbols as the case gives
them, raw bits for what is malformed); and the zlib framing for such a stream, with a header and an
Adler-32 that are right or deliberately wrong.  Pure Python + NumPy, no project code."""
import struct
import zlib
from typing import NamedTuple

import numpy as np

SIGNATURE = bytes([137, 80, 78, 71, 13, 10, 26, 10])


def chunk(typ: bytes, body: bytes = b"") -> bytes:
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def _paeth(a, b, c):
    """PNG's Paeth predictor on int arrays (or ints)."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


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
            pred = _paeth(left, up, upleft)
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


def zlib_wrap(raw_deflate: bytes, data: bytes, adler_delta: int = 0, cmf: int = 0x78, flg=None, adler_bytes: int = 4) -> bytes:
    """CMF FLG | a hand-written deflate stream | the first adler_bytes bytes of the Adler-32 of data
    (plus adler_delta).  flg None: FLEVEL 0, no FDICT, the FCHECK that makes the header right (78 01)."""
    if flg is None:
        flg = (31 - (cmf << 8) % 31) % 31
    return bytes([cmf, flg]) + raw_deflate + struct.pack(">I", (zlib.adler32(data) + adler_delta) & 0xFFFFFFFF)[:adler_bytes]


class BitWriter:
    """Deflate's bit order: values LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0  # the bits of the unfinished byte
        self.n = 0    # how many

    def put(self, value: int, n: int):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code: int, n: int):
        return self.put(int(format(code, f"0{n}b")[::-1], 2), n) if n else self

    def fixed_literal(self, v: int):
        return self.code(0x30 + v, 8) if v < 144 else self.code(0x190 + v - 144, 9)

    def align(self):
        """Zero bits up to the next byte boundary."""
        return self.put(0, -self.n % 8)

    def raw(self, data: bytes):
        assert self.n == 0, "raw bytes go on a byte boundary"
        self.out += data
        return self

    def bit_length(self) -> int:
        return 8 * len(self.out) + self.n

    def bytes(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canonical_codes(lengths):
    """symbol -> its canonical code (RFC 1951 3.2.2) for the given lengths, None where the length is 0.
    The set may be incomplete; an over-subscribed one gets codes that no longer fit their lengths."""
    count = [0] * 16
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for ln in range(1, 16):
        code = (code + count[ln - 1]) << 1
        nxt[ln] = code
    out = []
    for ln in lengths:
        out.append(nxt[ln] if ln else None)
        nxt[ln] += 1 if ln else 0
    return out


class Raw(NamedTuple):
    """A token that is written as it stands: `bits` bits of `code`, MSB first like a Huffman code."""
    code: int
    bits: int


def default_cl_lens(used):
    """A complete code-length code over the symbols `used`: lengths L - 1 and L (two symbols at the
    least, since zlib refuses an incomplete code-length code)."""
    used = sorted(set(used))
    for extra in (0, 18, 17):
        if len(used) < 2 and extra not in used:
            used = sorted(used + [extra])
    k = len(used)
    L = max(1, (k - 1).bit_length())
    short = (1 << L) - k
    lens = [0] * 19
    for j, s in enumerate(used):
        lens[s] = L - 1 if j < short else L
    return lens


class Deflate:
    """A deflate stream written block by block into ONE bit stream: a block's header bits follow the
    end-of-block code of the block before in the same byte.  Tokens are int literals, (length,
    distance) matches, (length, distance, length symbol) to force the length symbol (258 as symbol
    284 + extra 31), or Raw bits.  Nothing is checked that a malformed case may want to violate."""

    def __init__(self):
        self.w = BitWriter()

    def bytes(self) -> bytes:
        return self.w.bytes()

    def stored(self, data: bytes, final: bool = False, length=None):
        """length: the LEN field when it is not to be len(data) (NLEN is its complement)."""
        n = len(data) if length is None else length
        assert 0 <= n <= 65535
        self.w.put(int(final), 1).put(0, 2).align().put(n, 16).put(n ^ 0xFFFF, 16).raw(bytes(data))
        return self

    def _tokens(self, tokens, lit_lens, dist_lens, eob):
        lit, dist = canonical_codes(lit_lens), canonical_codes(dist_lens)
        w = self.w
        for t in tokens:
            if isinstance(t, Raw):
                w.code(t.code, t.bits)
            elif isinstance(t, int):
                assert lit_lens[t], f"literal {t} has no code"
                w.code(lit[t], lit_lens[t])
            else:
                length, distance = t[0], t[1]
                ls = t[2] - 257 if len(t) > 2 else max(k for k in range(29) if LEN_BASE[k] <= length)
                assert 0 <= length - LEN_BASE[ls] < (1 << LEN_EXTRA[ls]) or length == LEN_BASE[ls]
                ds = max(k for k in range(30) if DIST_BASE[k] <= distance)
                assert lit_lens[257 + ls] and dist_lens[ds], f"match {t} has no code"
                w.code(lit[257 + ls], lit_lens[257 + ls]).put(length - LEN_BASE[ls], LEN_EXTRA[ls])
                w.code(dist[ds], dist_lens[ds]).put(distance - DIST_BASE[ds], DIST_EXTRA[ds])
        if eob:
            w.code(lit[256], lit_lens[256])

    def fixed(self, tokens, final: bool = False, eob: bool = True):
        self.w.put(int(final), 1).put(1, 2)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST, eob)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final: bool = False, cl_symbols=None, hclen=None, cl_lens=None, eob: bool = True):
        """lit_lens / dist_lens: the HLIT = len(lit_lens) and HDIST = len(dist_lens) code lengths as
        they are to be used for the tokens.  cl_symbols: the (symbol, extra) code-length symbols that
        write them (default: one symbol 0..15 per length, no repeats) -- what they spell is the case's
        business.  cl_lens: the 19 lengths of the code-length code (default: a complete code over the
        symbols used).  hclen: how many of them are sent (default: the least that holds them)."""
        hlit, hdist = len(lit_lens), len(dist_lens)
        if cl_symbols is None:
            cl_symbols = [(ln, 0) for ln in list(lit_lens) + list(dist_lens)]
        if cl_lens is None:
            cl_lens = default_cl_lens(s for s, _ in cl_symbols)
        if hclen is None:
            hclen = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
        w = self.w
        w.put(int(final), 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
        for k in range(hclen):
            w.put(cl_lens[CL_ORDER[k]], 3)
        cl = canonical_codes(cl_lens)
        for s, extra in cl_symbols:
            assert cl_lens[s], f"code-length symbol {s} has no code"
            w.code(cl[s], cl_lens[s]).put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))
        self._tokens(tokens, lit_lens, dist_lens, eob)
        return self


def inflate_tokens(tokens) -> bytes:
    """What a token list (literals and matches) spells."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def tokens_of(data: bytes, start: int, stop: int, matches=()):
    """data[start:stop] as literals, except that each (at, length, distance[, length symbol]) of
    matches is sent as that match -- which data must really contain."""
    by_at = {m[0]: m for m in matches}
    out, i = [], start
    while i < stop:
        m = by_at.get(i)
        if m:
            assert i + m[1] <= stop and all(data[i + k] == data[i + k - m[2]] for k in range(m[1])), f"no such match: {m}"
            out.append(tuple(m[1:]))
            i += m[1]
        else:
            out.append(data[i])
            i += 1
    assert i == stop
    return out
