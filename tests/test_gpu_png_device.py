"""The device PNG writer (csrc/nic_png_dev.hip; DESIGN.md "The device PNG writer") on the GPU:
its files are valid PNGs (tests/png_parse.py checks the framing and every CRC, zlib the deflate
stream and the Adler-32, Pillow the pixels), the adaptive filter choice is Pillow's, the code-length
limit, degenerate and incompressible blocks, determinism and batch invariance, the file size
against zlib's Huffman-only coder, and the directory drivers with png_writer="device"."""
import ctypes
import heapq
import io
import os
import shutil
import zlib

import numpy as np
import pytest

from tests import png_parse as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import _lib  # noqa: E402
from neural_network_image_compression_amd import bitstream as B  # noqa: E402
from neural_network_image_compression_amd.codec import Codec, Decoder, Encoder  # noqa: E402

BLOCK = _lib.lib().nic_png_device_block_bytes()
# a block's largest cost beside its symbols, in bits: BFINAL/BTYPE, HLIT/HDIST/HCLEN, the 19 lengths
# of the code-length code, 258 code lengths of at most 7 bits, and the empty stored block that
# realigns (3 header bits, up to 7 padding bits, LEN and NLEN)
BLOCK_OVERHEAD = (3 + 14 + 19 * 3 + 258 * 7 + 3 + 7 + 32 + 7) // 8
TRAINED = ("kodim21_256_trained", "kodim21_256_trained_c0.02", "kodim21_256_trained_c0.03", "imagenet4_trained",
           "imagenet4_trained_c0.02", "imagenet4_trained_c0.03")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def codec():
    c = Codec(0)  # the writer needs no weights
    yield c
    c.close()


def bound(h, w, c):
    b = ctypes.c_int64()
    assert _lib.lib().nic_png_device_bound(h, w, c, ctypes.byref(b)) == _lib.NIC_OK
    return b.value


def encode(codec, x, filter="adaptive", stride=None):
    """The files of x (N,H,W,C) as bytes, from the raw buffers: sizes[i] is the file's length and
    nothing past it is read."""
    buf, sizes = codec.png_encode(_dev(x), filter, stride=stride)
    buf, sizes = buf.cpu().numpy(), sizes.cpu().numpy()
    n, h, w, c = x.shape
    assert buf.shape == (n, stride if stride is not None else bound(h, w, c)) and sizes.shape == (n,)
    assert (sizes > 0).all() and (sizes <= bound(h, w, c)).all()
    return [buf[i, :sizes[i]].tobytes() for i in range(n)]


def check_file(data, img):
    """Framing, CRCs, IHDR, Adler-32 (png_parse), exactly the chunks of the format, and Pillow's
    decoded pixels.  Returns the parsed file."""
    from PIL import Image

    h, w, c = img.shape
    png = P.parse(data)  # asserts that the file ends with IEND: sizes[i] is its true length
    assert [t for t, _ in png.chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert (png.width, png.height, png.bit_depth, png.colour_type, png.interlace) == (w, h, 8, 2 if c == 3 else 0, 0)
    assert png.idat[0] == 0x78 and (png.idat[0] * 256 + png.idat[1]) % 31 == 0
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == ("RGB" if c == 3 else "L")
        np.testing.assert_array_equal(np.array(im).reshape(h, w, c), img)
    return png


def pillow_filtered(img):
    """The filtered stream inside Pillow's optimize=True file of img (H,W,C)."""
    return P.parse(B.png_bytes(img[:, :, 0] if img.shape[2] == 1 else img)).filtered


def smooth(rng, shape):
    """Random-walk images: neighbouring pixels are close, so the five filters differ."""
    a = np.cumsum(rng.integers(-3, 4, shape), axis=2) + np.cumsum(rng.integers(-2, 3, shape), axis=1)
    return (a % 256).astype(np.uint8)


def _conformance_inputs(golden):
    rng = np.random.default_rng(11)
    rows2 = 2 * BLOCK // 256  # 1-channel rows of 255 pixels: 256 filtered bytes each
    cases = {
        "1x1": rng.integers(0, 256, (1, 1, 1, 3), dtype=np.uint8),
        "1x7": smooth(rng, (1, 1, 7, 3)),
        "5x1": smooth(rng, (1, 5, 1, 3)),
        "8x8": smooth(rng, (2, 8, 8, 3)),
        "37x53 grey": smooth(rng, (3, 37, 53, 1)),
        "odd37x53 recon": golden("odd37x53")["recon"],
        "kodim21 trained recon": golden("kodim21_256_trained")["recon"],
        "two blocks exactly": smooth(rng, (1, rows2, 255, 1)),
        "two blocks and a row": smooth(rng, (1, rows2 + 1, 255, 1)),
    }
    assert cases["odd37x53 recon"].shape == (1, 40, 56, 3) and cases["kodim21 trained recon"].shape[1:] == (256, 256, 3)
    assert rows2 * 256 == 2 * BLOCK
    return cases


@pytest.mark.parametrize("case", ["1x1", "1x7", "5x1", "8x8", "37x53 grey", "odd37x53 recon", "kodim21 trained recon",
                                  "two blocks exactly", "two blocks and a row"])
def test_conformance(codec, golden, case):
    x = _conformance_inputs(golden)[case]
    n, h, w, c = x.shape
    files = encode(codec, x)
    for i, data in enumerate(files):
        png = check_file(data, x[i])
        assert png.filtered == pillow_filtered(x[i]), f"image {i}: the filtered stream is not Pillow's"
        blocks = P.deflate_blocks(png.idat)
        nblocks = (h * (w * c + 1) + BLOCK - 1) // BLOCK
        data_blocks = [b for b in blocks if not (b["type"] == "stored" and b["symbols"] == 0)]
        assert len(data_blocks) == nblocks and all(b["symbols"] <= BLOCK for b in data_blocks)
        assert sum(b["symbols"] for b in data_blocks) == h * (w * c + 1)
        assert all(b["start_bit"] % 8 == 0 for b in data_blocks)  # blocks are concatenated as bytes
        assert all(b["max_len"] <= 15 for b in blocks if b["type"] == "dynamic")


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4])
def test_fixed_filters(codec, filt):
    rng = np.random.default_rng(12)
    for x in (smooth(rng, (2, 8, 8, 3)), smooth(rng, (3, 37, 53, 1))):
        for i, data in enumerate(encode(codec, x, filter=filt)):
            png = check_file(data, x[i])
            assert set(png.filter_bytes()) == {filt}


def huffman_depth(counts, deep):
    """Depth of an unlimited Huffman tree on counts (> 0); ties go to the deeper (deep) or the
    shallower subtree."""
    heap = [(c, 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        d = max(abs(a[1]), abs(b[1])) + 1
        heapq.heappush(heap, (a[0] + b[0], -d if deep else d))
    return abs(heap[0][1])


def test_code_length_limit(codec):
    """The first block's symbols have the Fibonacci counts 1, 1, 2, 3, 5, ..., 2584: the first 1 is
    the end-of-block code, the other 17 are byte values (a second byte value of count 1 beside the
    end-of-block code would tie, and the ties admit an optimal tree of depth 11); the rest of the
    block is one padding value.  Every optimal unlimited Huffman code is then 18 bits deep."""
    w, rows = 255, BLOCK // 256
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) == 6764
    counts = {v: fib[v + 1] for v in range(17)}  # value 0 takes the largest count below
    counts[0], counts[16] = fib[17], fib[1]
    assert counts[0] > rows
    body = []
    for v, c in counts.items():
        body += [v] * (c - rows if v == 0 else c)  # the block also holds one filter byte 0 per row
    pad = rows * w - len(body)
    body += [255] * pad
    block_counts = sorted(list(fib) + [pad])
    assert sum(block_counts) == BLOCK + 1
    assert huffman_depth(block_counts, deep=False) > 15 and huffman_depth(block_counts, deep=True) > 15
    first = np.random.default_rng(13).permutation(np.array(body, np.uint8)).reshape(rows, w)
    x = np.concatenate([first, np.full((6, w), 255, np.uint8)])[None, :, :, None]
    data, = encode(codec, x, filter=0)
    png = check_file(data, x[0])
    blocks = P.deflate_blocks(png.idat)
    assert blocks[0]["type"] == "dynamic" and blocks[0]["symbols"] == BLOCK and blocks[0]["max_len"] <= 15


@pytest.mark.parametrize("value", [0, 255])
def test_degenerate_blocks_and_checksum_wrap(codec, value):
    x = np.full((1, 64, 4096, 1), value, np.uint8)
    data, = encode(codec, x, filter=0)
    png = check_file(data, x[0])
    assert len(data) < x.size // 4  # one or two bits per byte
    blocks = [b for b in P.deflate_blocks(png.idat) if b["symbols"]]
    assert all(b["type"] == "dynamic" and b["max_len"] <= 2 for b in blocks)


@pytest.mark.parametrize("shape", [(1, 64, 4096, 1), (1, 33, 100, 3)])
def test_incompressible(codec, shape):
    g = torch.Generator().manual_seed(14)
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).numpy()
    data, = encode(codec, x, filter=0)
    n, h, w, c = shape
    assert len(data) <= bound(h, w, c)
    png = check_file(data, x[0])
    blocks = P.deflate_blocks(png.idat)
    total = h * (w * c + 1)
    big = [b for b in blocks if b["symbols"] >= 4096]
    assert len(big) == max(1, total // BLOCK) and all(b["type"] == "stored" for b in big)  # 8 bits per byte: no gain


def test_determinism_and_batch_invariance(codec):
    rng = np.random.default_rng(15)
    x = smooth(rng, (5, 16, 24, 3))
    files = encode(codec, x)
    assert len(set(files)) == 5
    assert encode(codec, x[3:4]) == [files[3]]
    assert encode(codec, x) == files
    wide = bound(16, 24, 3) + 333
    assert encode(codec, x, stride=wide) == files
    for i, data in enumerate(files):
        check_file(data, x[i])
    # the workspace is reused: another shape in between changes nothing
    encode(codec, smooth(rng, (2, 40, 31, 1)))
    assert encode(codec, x) == files


def test_size_against_zlib_huffman_only(codec, golden):
    """Both sides are optimal prefix coders of literals, so the device IDAT may exceed zlib's
    Z_HUFFMAN_ONLY stream of the same filtered bytes by the blocks' header and alignment cost only."""
    for name in TRAINED:
        recon = golden(name)["recon"]
        for i, data in enumerate(encode(codec, recon)):
            png = check_file(data, recon[i])
            co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
            ref = len(co.compress(png.filtered) + co.flush())
            pil = len(P.parse(B.png_bytes(recon[i])).idat)
            nblocks = (len(png.filtered) + BLOCK - 1) // BLOCK
            print(f"{name}[{i}]: filtered {len(png.filtered)} device IDAT {len(png.idat)} zlib huffman-only {ref} "
                  f"pillow {pil} device/pillow {len(png.idat) / pil:.4f} blocks {nblocks}")
            assert len(png.idat) <= ref + nblocks * BLOCK_OVERHEAD


def test_drivers_with_the_device_writer(tmp_path, golden, weights_trained):
    from PIL import Image

    from neural_network_image_compression_amd import weights as W
    ds = tmp_path / "imgs"
    ds.mkdir()
    g = golden("imagenet4")
    names = ["a0", "a1", "a2", "a3", "b"]
    imgs = [np.ascontiguousarray(g["x"][i][32:48, 16:32]) for i in range(4)] + [np.ascontiguousarray(g["x"][0][8:32, 8:16])]
    assert imgs[0].shape == (16, 16, 3) and imgs[4].shape == (24, 8, 3)
    for name, a in zip(names, imgs):
        Image.fromarray(a).save(ds / f"{name}.png")
    W.save(weights_trained, str(tmp_path / "ck" / "encoder"), "encoder")
    W.save(weights_trained, str(tmp_path / "ck" / "decoder"), "decoder")
    enc, dec = Encoder(0), Decoder(0)
    with pytest.raises(ValueError, match="png_writer"):
        dec.uncompress(str(tmp_path / "imgs_compressed"), str(tmp_path / "ck" / "decoder"), png_writer="gpu")
    for container in B.CONTAINERS:
        enc.compress(str(ds), str(tmp_path / "ck" / "encoder"), container=container)
        comp = tmp_path / f"{container}dev_compressed"
        shutil.copytree(tmp_path / "imgs_compressed", comp)
        dec.uncompress(str(tmp_path / "imgs_compressed"), str(tmp_path / "ck" / "decoder"), container=container)
        dec.uncompress(str(comp), str(tmp_path / "ck" / "decoder"), container=container, png_writer="device")
        default, device = tmp_path / "imgs_uncompressed", tmp_path / f"{container}dev_uncompressed"
        assert sorted(os.listdir(device)) == sorted(os.listdir(default)) == [n + ".png" for n in names]
        for n, a in zip(names, imgs):
            rec = dec.codec.decode(enc.codec.encode(_dev(a[None]))).cpu().numpy()
            # the default writer's files are untouched: Pillow's bytes of the reconstruction
            assert (default / f"{n}.png").read_bytes() == B.png_encode(rec)[0], n
            png = check_file((device / f"{n}.png").read_bytes(), rec[0])
            assert png.filtered == pillow_filtered(rec[0])
            with Image.open(default / f"{n}.png") as p0, Image.open(device / f"{n}.png") as p1:
                np.testing.assert_array_equal(np.array(p0), np.array(p1))
        shutil.rmtree(tmp_path / "imgs_compressed")
        shutil.rmtree(default)
    # the serial driver takes the same route
    enc.compress(str(ds), str(tmp_path / "ck" / "encoder"))
    dec.uncompress(str(tmp_path / "imgs_compressed"), str(tmp_path / "ck" / "decoder"), workers=0, batch_size=2,
                   png_writer="device")
    for n in names:
        assert (tmp_path / "imgs_uncompressed" / f"{n}.png").read_bytes() == \
            (tmp_path / "pngdev_uncompressed" / f"{n}.png").read_bytes(), n
