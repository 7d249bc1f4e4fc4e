"""Writes the corpus of tools/png_read_host_check.cpp: one file per zlib stream,
u32 T | u8 expect | u8 status | u8 bytes | [T bytes] | stream, where expect is 0 iff zlib.decompress
returns exactly T bytes, status is the exact status the stream must give (its bits 1, 2, 4 and 8: the
filter bit is not inflate's; 255 where only zlib's verdict is known) and the T bytes, present for every
stream zlib takes, are zlib's output.

  python tools/png_read_corpus.py OUT_DIR

The streams: every file of tests/test_png_read_format.py (Pillow's, the native writer's in both modes,
tests/png_make.py's), the status cases of tests/test_gpu_png_read.py, the edge streams of
tests/png_read_cases.py (hand-written deflate that zlib takes but never writes, and one defect each
for the refused ones), every truncation length of the 3x5 file's stream and every single-bit flip of
the first 4,096 bits of the 37x53 file's stream."""
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_parse, png_read_cases as C  # noqa: E402

UNPINNED = 255


def judge(stream: bytes, T: int):
    """(expect, zlib's bytes when it returns exactly T of them)."""
    try:
        data = zlib.decompress(stream)
    except zlib.error:
        return 1, None
    return (0, data) if len(data) == T else (1, None)


def items():
    """[(name, stream, T, status or UNPINNED)]"""
    out = []
    for name, data in C.format_files().items():
        p = png_parse.parse(data)
        out.append((name, p.idat, len(p.filtered), 0))
    for name, (stream, T, status) in C.status_streams().items():
        out.append(("status_" + name, stream, T, status & 15))
    for name, (stream, (h, w, ch), status) in C.edge_streams().items():
        out.append(("edge_" + name, stream, h * (w * ch + 1), status))
    s35, T35 = C.stream_of(C.rgb_image(3, 5))
    for n in range(len(s35)):
        out.append((f"trunc_{n:03d}", s35[:n], T35, UNPINNED))
    s37, T37 = C.stream_of(C.rgb_image(37, 53))
    for bit in range(min(4096, 8 * len(s37))):
        b = bytearray(s37)
        b[bit >> 3] ^= 1 << (bit & 7)
        out.append((f"flip_{bit:04d}", bytes(b), T37, UNPINNED))
    return out


def write(out_dir: str):
    """-> (streams, of them taken by zlib, of them with an exact status)"""
    os.makedirs(out_dir, exist_ok=True)
    its = items()
    taken = pinned = 0
    for name, stream, T, status in its:
        e, data = judge(stream, T)
        taken += e == 0
        pinned += status != UNPINNED
        with open(os.path.join(out_dir, name + ".bin"), "wb") as f:
            f.write(struct.pack("<IBBB", T, e, status, data is not None) + (data or b"") + stream)
    return len(its), taken, pinned


def main(out_dir: str) -> None:
    n, taken, pinned = write(out_dir)
    print(f"{n} streams in {out_dir}: zlib takes {taken}, refuses {n - taken}; {pinned} with an exact status")


if __name__ == "__main__":
    main(sys.argv[1])
