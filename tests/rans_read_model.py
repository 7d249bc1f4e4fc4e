"""A lenient reader of .nic files, versions 1 to 3: what the device reader (nic_rans_decode,
nic_rans2_decode, nic_rans3_decode and their window forms) promises for ANY bytes, restated in plain
Python from include/nic.h and DESIGN.md ("The .nic container": the format, the status bits, "What
the device reader does with a malformed file").  tests/rans_ref.py and its siblings are strict
(they raise); this reader never raises: it returns the status word of nic.h and, for a status-0
file, the latent.  Nothing here touches the library.

The rules:
- the size is clamped to [0, stride]; a byte at or past it reads as 0;
- a header that is no header of this version and geometry gives bit 1, a foreign prior bit 3, and
  nothing is decoded;
- every stored table is checked against "symbols ascending, freqs in 1..4096, sum 4096" (bit 2), and
  its cumulative row is built so that every slot resolves (lenient_row);
- segment offsets are prefix sums of the stored lengths, saturating at the size;
- a segment is decoded with reads past its end as 0, at most two refill bytes per symbol, and sets
  bit 0 unless it ends at state 2^23 on its last byte.
"""
import numpy as np

from tests import rans2_ref as R2
from tests import rans3_ref as R3
from tests import rans_ref as R

CH, M, L = R.CH, R.M, R.L
HEADER = {1: 16, 2: 40, 3: 40}
BAD_SEGMENT, BAD_HEADER, BAD_TABLE, FOREIGN_PRIOR = 1, 2, 4, 8


def lenient_row(entries):
    """n (symbol, freq) entries as stored -> (start[0..256], broken).  The walk of DESIGN.md: s runs
    over 0..255 with run = 0 and a cursor at the first entry; start[s] = run; an entry whose symbol
    is s is consumed, run = min(run + freq, 4096); start[256] = 4096.  So start[0] = 0, the row never
    decreases and every slot in 0..4095 lies in exactly one [start[s], start[s + 1]).  broken: the
    table is not "symbols ascending, freqs in 1..4096, sum 4096"."""
    start, run, e = [], 0, 0
    broken = False
    for s in range(256):
        start.append(run)
        if e < len(entries) and entries[e][0] == s:
            f = entries[e][1]
            broken |= not 1 <= f <= M or run + f > M
            run = min(run + f, M)
            e += 1
    start.append(M)
    broken |= e != len(entries) or run != M  # an entry that is never reached: its symbol does not ascend
    return start, broken


def _row_of_freqs(freqs):
    return np.concatenate([[0], np.cumsum(np.asarray(freqs, np.int64))]).tolist()


def _lut(start):
    """slot -> the largest s with start[s] <= slot."""
    return (np.searchsorted(np.asarray(start[:256]), np.arange(M), side="right") - 1).tolist()


_PRIOR_ROWS = {}  # (ver, id(prior), channel) -> the prior's rows, built once per prior object


def _prior_rows(ver, prior, c):
    key = (ver, id(prior), c)
    if key not in _PRIOR_ROWS:
        starts = [_row_of_freqs(prior[c])] if ver == 2 else [_row_of_freqs(f) for f in prior[1][c]]
        _PRIOR_ROWS[key] = (prior, [(s, _lut(s)) for s in starts])  # the prior is kept alive with its key
    return _PRIOR_ROWS[key][1]


def _decode(ver, data, size, h8, w8, prior, stride):
    """-> (bits 1 to 3 of the status, the set of segments that set bit 0, the decoded symbols)."""
    data = bytes(data)
    stride = len(data) if stride is None else stride
    size = max(0, min(int(size), stride, len(data), 0x7FFFFFFF))
    hdr = HEADER[ver]

    def rd(i):
        return data[i] if i < size else 0

    def rd32(i):
        return rd(i) | rd(i + 1) << 8 | rd(i + 2) << 16 | rd(i + 3) << 24

    S = rd(6) | rd(7) << 8
    ok = (size >= hdr and bytes(rd(i) for i in range(4)) == R.MAGIC and rd(4) == ver and rd(5) == R.PROB_BITS and S >= 1
          and rd32(8) == h8 and rd32(12) == w8)
    if ok and ver != 1:
        ok = -(-rd32(16) // 8) == h8 and -(-rd32(20) // 8) == w8
    if not ok:
        return BAD_HEADER, set(), None
    anchors = None
    if ver == 2 and rd32(24) != R2.prior_id(prior):
        return FOREIGN_PRIOR, set(), None
    if ver == 3:
        if rd32(24) != R3.prior_id(prior):
            return FOREIGN_PRIOR, set(), None
        anchors = [int(a) for a in prior[0]]
    status = 0
    # rows[c][k]: (start, lut) of channel c in context k (one context before version 3)
    nctx = 3 if ver == 3 else 1
    rows, at = [], hdr
    for c in range(CH):
        if ver != 1 and not (rd(28 + (c >> 3)) >> (c & 7)) & 1:
            rows.append(_prior_rows(ver, prior, c))
            continue
        n = rd(at) + 1
        entries = [(rd(at + 1 + 3 * e), rd(at + 2 + 3 * e) | rd(at + 3 + 3 * e) << 8) for e in range(n)]
        start, broken = lenient_row(entries)
        if broken:
            status |= BAD_TABLE
        rows.append([(start, _lut(start))] * nctx)
        at += 1 + 3 * n
    npix = h8 * w8
    nseg = -(-npix // S)
    pay = min(at + 4 * nseg, size)
    off = [0]
    for k in range(nseg):
        off.append(min(off[-1] + rd32(at + 4 * k), size))
    out, failing = [], set()
    for k in range(nseg):
        ptr, end = min(pay + off[k], size), min(pay + off[k + 1], size)
        x = 0
        for _ in range(4):  # the segment's leading big-endian final state
            x = x << 8 | (data[ptr] if ptr < end else 0)
            ptr += 1
        seg = []
        for j in range(CH * min(S, npix - k * S)):
            c = j % CH
            kx = 0 if ver != 3 or j < CH else min(2, abs(seg[j - CH] - anchors[c]))
            start, lut = rows[c][kx]
            slot = x & (M - 1)
            s = lut[slot]
            x = (start[s + 1] - start[s]) * (x >> R.PROB_BITS) + slot - start[s]
            for _ in range(2):  # at most two refill bytes per symbol
                if x < L:
                    x = x << 8 | (data[ptr] if ptr < end else 0)
                    ptr += 1
            seg.append(s)
        if x != L or ptr != end:
            failing.add(k)
        out += seg
    return status, failing, out


def read(ver, data, size, h8, w8, prior=None, stride=None):
    """The slot's bytes `data`, the size passed for it (clamped to [0, min(stride, len(data))]), the
    call's (h8, w8) and the codec's prior (version 2: 96 x 256 freqs; version 3: (anchors, 96 x 3 x
    256 freqs)) -> (status, latent (h8, w8, 96) u8 or None).  The latent is None unless the status is
    0: an image with a non-zero status may hold anything inside its own bytes."""
    status, failing, out = _decode(ver, data, size, h8, w8, prior, stride)
    if failing:
        status |= BAD_SEGMENT
    if status:
        return status, None
    return 0, np.array(out, dtype=np.uint8).reshape(h8, w8, CH)


def window_status(ver, data, size, h8, w8, window, prior=None, stride=None):
    """The status of a window decode (nic_rans*_decode_window, nic_rans*_decode_windows): bits 1, 2
    and 3 as in read(); bit 0 covers only the segments that hold a pixel of window = (r0, c0, rows,
    cols)."""
    status, failing, _ = _decode(ver, data, size, h8, w8, prior, stride)
    if failing:
        S = data[6] | data[7] << 8
        r0, c0, nr, nc = window
        if failing & {((r0 + i) * w8 + c0 + x) // S for i in range(nr) for x in range(nc)}:
            status |= BAD_SEGMENT
    return status
