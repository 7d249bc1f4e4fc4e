"""Writes the corpus of tools/png_read_host_check.cpp: one file per zlib stream,
u32 T | u8 expect | stream, where expect is 0 iff zlib.decompress returns exactly T bytes.

  python tools/png_read_corpus.py OUT_DIR

The streams: every file of tests/test_png_read_format.py (Pillow's, the native writer's in both modes,
tests/png_make.py's), the status cases of tests/test_gpu_png_read.py, every truncation length of the
3x5 file's stream and every single-bit flip of the first 4,096 bits of the 37x53 file's stream."""
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_parse, png_read_cases as C  # noqa: E402


def expect(stream: bytes, T: int) -> int:
    try:
        return 0 if len(zlib.decompress(stream)) == T else 1
    except zlib.error:
        return 1


def main(out_dir: str) -> None:
    os.makedirs(out_dir, exist_ok=True)
    items = []
    for name, data in C.format_files().items():
        p = png_parse.parse(data)
        items.append((name, p.idat, len(p.filtered)))
    for name, (stream, T, _) in C.status_streams().items():
        items.append(("status_" + name, stream, T))
    s35, T35 = C.stream_of(C.rgb_image(3, 5))
    for n in range(len(s35)):
        items.append((f"trunc_{n:03d}", s35[:n], T35))
    s37, T37 = C.stream_of(C.rgb_image(37, 53))
    for bit in range(min(4096, 8 * len(s37))):
        b = bytearray(s37)
        b[bit >> 3] ^= 1 << (bit & 7)
        items.append((f"flip_{bit:04d}", bytes(b), T37))
    refused = 0
    for name, stream, T in items:
        e = expect(stream, T)
        refused += e
        with open(os.path.join(out_dir, name + ".bin"), "wb") as f:
            f.write(struct.pack("<IB", T, e) + stream)
    print(f"{len(items)} streams in {out_dir}: zlib takes {len(items) - refused}, refuses {refused}")


if __name__ == "__main__":
    main(sys.argv[1])
