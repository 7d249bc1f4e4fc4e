"""The device PNG reader on the GPU: Codec.png_read against Pillow's pixels, byte for byte, over the
block types, filters, window distances and writers; deflate's edges that zlib never writes (the edge
streams of tests/png_read_cases.py: matches whose source and destination share slots of the 32 KB LDS
ring, codes longer than the fast table, header forms, block sequences, headers on the input ring's
first restage); unfilter at the widest rows; the status bits, with nothing stored outside the images;
the drivers with png_reader="device" against the "pillow" run's files.  Every hand-made stream here
goes through tools/png_read_host_check.cpp (the same nic_inflate.h on the CPU, under sanitizers) in
tests/test_png_inflate_host.py first, which also proves that each reaches its edge."""
import io
import os
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_make as M
from tests import png_parse, png_read_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def codec():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neural_network_image_compression_amd.codec import Codec

    return Codec(0)


def pillow_pixels(data: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        a = np.array(im)
    return a if a.ndim == 3 else a[:, :, None]


def read_streams(codec, streams, h, w, ch):
    from neural_network_image_compression_amd import bitstream as B

    buf, lens = B._upload_files(codec, [s if s else b"\0" for s in streams])
    if any(len(s) == 0 for s in streams):
        lens = lens * 0 + lens.new_tensor([len(s) for s in streams])
    return codec.png_read_status(buf, lens, h, w, ch)


def read_files(codec, files):
    from neural_network_image_compression_amd import bitstream as B

    parts = [B.png_stream(f) for f in files]
    h, w, ch = parts[0][:3]
    assert all(p[:3] == (h, w, ch) for p in parts)
    return read_streams(codec, [p[3] for p in parts], h, w, ch)


def check_files(codec, files):
    import torch

    images, status = read_files(codec, files)
    assert status.cpu().tolist() == [0] * len(files)
    want = torch.from_numpy(np.stack([pillow_pixels(f) for f in files])).to(images.device)
    assert torch.equal(images, want)
    return images


def test_one_pixel_files_are_fixed_huffman(codec):
    for a in (np.array([[[7, 130, 255]]], np.uint8), np.array([[201]], np.uint8)):
        data = C.pillow_png(a, optimize=True)
        assert [b["type"] for b in png_parse.deflate_blocks(png_parse.parse(data).idat)] == ["fixed"]
        check_files(codec, [data])


@pytest.mark.parametrize("h,w", [(1, 9), (9, 1), (3, 5), (37, 53)])
def test_small_and_odd_shapes(codec, h, w):
    a = C.rgb_image(h, w)
    check_files(codec, [C.pillow_png(a, optimize=True)])
    check_files(codec, [M.make_png(a, [r % 5 for r in range(h)][::-1])])  # a first row with every filter in turn
    check_files(codec, [M.make_png(a, f) for f in range(5)])


def test_every_filter_on_a_natural_crop(codec):
    a = C.rgb_image(64, 64)
    files = [M.make_png(a, f, level=9) for f in range(5)] + [C.pillow_png(a, optimize=True)]
    for f in range(5):
        assert set(png_parse.parse(files[f]).filter_bytes()) == {f}
    assert len(set(png_parse.parse(files[5]).filter_bytes())) >= 2  # the adaptive file mixes filters
    check_files(codec, files)


def test_two_stored_blocks(codec):
    a = np.ascontiguousarray(np.tile(C.rgb_image(75, 75), (2, 2, 1)))
    data = M.make_png(a, 0, level=0)
    blocks = png_parse.deflate_blocks(png_parse.parse(data).idat)
    assert [b["type"] for b in blocks] == ["stored", "stored"] and sum(b["symbols"] for b in blocks) == 67650
    check_files(codec, [data])


def test_overlapping_matches_of_length_258(codec):
    a = np.full((96, 96, 3), 77, np.uint8)
    data = M.make_png(a, 0, level=9)
    assert len(png_parse.parse(data).idat) < 200
    check_files(codec, [data])


def test_far_window_and_small_window(codec):
    """The 32 KB window's stream reaches the repeat at distance 18,496; the 512-byte window's cannot go
    beyond 250 (the window less zlib's 262-byte lookahead) and is more than twice as long.  (The walker
    could not walk these streams while it dropped the bits of every distance code: `pos += f(pos)`
    reads pos before f moves it.)"""
    top = C.rgb_image(64, 96)
    a = np.ascontiguousarray(np.concatenate([top, top]))  # rows 64..127 repeat rows 0..63: distance 64 * 289 = 18,496
    far, near = M.make_png(a, 0, level=9), M.make_png(a, 0, level=9, wbits=9)
    zf, zn = png_parse.parse(far).idat, png_parse.parse(near).idat
    assert zf[0] >> 4 == 7 and zn[0] >> 4 == 1
    assert zf[2:] != zn[2:] and 2 * len(zf) < len(zn)
    bf, bn = png_parse.deflate_blocks(zf), png_parse.deflate_blocks(zn)
    assert max(b["max_dist"] for b in bf) == 18496 and sum(len(b["far"]) for b in bf) > 0
    assert max(b["max_dist"] for b in bn) == 250 and len(bn) > len(bf)
    check_files(codec, [far, near])


# ---- deflate's edges (tests/png_read_cases.py edge_streams) -----------------------------------------
def edge_files(names):
    return [M.frame(*C.edge_streams()[n][1], C.edge_streams()[n][0]) for n in names]


def edge_groups():
    """shape -> the accepted edge streams' names of that shape"""
    groups = {}
    for name, (_, shape, status) in sorted(C.edge_streams().items()):
        if status == 0:
            groups.setdefault(shape, []).append(name)
    return groups


@pytest.mark.parametrize("shape", [C.FAR_SHAPE, C.SMALL_SHAPE, C.BIG_SHAPE], ids=["far", "small", "big"])
def test_edge_streams_are_read_as_pillow_reads_them(codec, shape):
    """One batch per shape: the far-distance matches (FAR_SHAPE), the long codes, header forms, block
    sequences and restage positions (SMALL_SHAPE), the 65,535-byte stored block (BIG_SHAPE)."""
    import torch

    names = edge_groups()[shape]
    assert len(names) == {C.FAR_SHAPE: 19, C.SMALL_SHAPE: 30, C.BIG_SHAPE: 1}[shape]
    images = check_files(codec, edge_files(names))
    want = np.stack([C.edge_image(n) for n in names])[..., None]  # zlib's bytes, as the CPU check compared them
    assert torch.equal(images.cpu(), torch.from_numpy(want))


def test_far_matches_do_not_depend_on_the_batch(codec):
    """The far-distance group again with a short stream (a flat image, under 200 bytes) on either side of
    every member: the same pixels as in the batch of their own."""
    import torch

    names = edge_groups()[C.FAR_SHAPE]
    h, w, _ = C.FAR_SHAPE
    flat = M.make_png(np.full((h, w), 9, np.uint8), 0, level=9)
    assert len(png_parse.parse(flat).idat) < 200
    alone = check_files(codec, edge_files(names))
    files = [flat]
    for f in edge_files(names):
        files += [f, flat]
    mixed = check_files(codec, files)
    assert torch.equal(mixed[1::2], alone) and bool((mixed[0::2] == 9).all())


def test_refused_edge_streams_give_their_status_and_touch_nothing_else(codec):
    """[good, bad, good, bad, ..., good] in one batch: every bad stream gives exactly its status, every
    good image is intact, and nothing is stored outside the images tensor."""
    import torch

    h, w, ch = C.SMALL_SHAPE
    names = sorted(n for n, v in C.edge_streams().items() if v[2] != 0)
    assert len(names) == 27 and all(C.edge_streams()[n][1] == C.SMALL_SHAPE for n in names)
    a = C.edge_image("twelve_blocks")
    good = C.edge_streams()["twelve_blocks"][0]
    streams, want = [good], [0]
    for n in names:
        streams += [C.edge_streams()[n][0], good]
        want += [C.edge_streams()[n][2], 0]
    count, pad = len(streams) * h * w * ch, 1 << 16
    big = torch.full((pad + count + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    out = big[pad:pad + count].view(len(streams), h, w, ch)
    from neural_network_image_compression_amd import bitstream as B

    buf, lens = B._upload_files(codec, [s if s else b"\0" for s in streams])
    lens = lens.new_tensor([len(s) for s in streams])
    images, status = codec.png_read_status(buf, lens, h, w, ch, out=out)
    assert images.data_ptr() == out.data_ptr()
    got = dict(zip(names, status.cpu().tolist()[1::2]))
    assert got == {n: C.edge_streams()[n][2] for n in names}
    assert status.cpu().tolist() == want
    good_px = torch.from_numpy(a[..., None]).cuda()
    assert all(torch.equal(out[k], good_px) for k in range(0, len(streams), 2))
    assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + count:] == 0xA5).all())


# ---- unfilter at the widest rows ----------------------------------------------------------------
def band_filters(h):
    """Rows 63, 64, 65, 127 and 128 take Paeth, Average, Up, Paeth and Average: row 64 k is lane 0 of a
    band and reads the row above through LDS."""
    return [(4, 3, 2, 1)[(r - 63) % 4] for r in range(h)]


@pytest.mark.parametrize("w,ch", [(16384, 1), (5461, 3)], ids=["grey16384", "rgb5461"])
@pytest.mark.parametrize("h", [65, 129])
def test_unfilter_at_the_widest_rows(codec, h, w, ch):
    """Rows of 16,384 and 16,383 bytes: the whole of uprow, which is indexed by mask.  Noise, so that
    every predictor's choice matters; with h = 129 and one channel also an all-255 image under filter
    0 (T = 2,113,665 bytes of which 2,113,536 are 255: both Adler sums wrap many times)."""
    rng = np.random.default_rng(h * 7 + ch)
    a = rng.integers(0, 256, (h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
    fs = band_filters(h)
    assert all(fs[r] == f for r, f in {63: 4, 64: 3, 65: 2, 127: 4, 128: 3}.items() if r < h) and len(fs) == h
    files = [M.make_png(a, fs, level=1)]
    got = png_parse.parse(files[0])
    assert list(got.filter_bytes()) == fs and got.width * got.channels == w * ch >= 16383
    if h == 129 and ch == 1:
        files.append(M.make_png(np.full((h, w), 255, np.uint8), 0, level=1))
        assert len(png_parse.parse(files[1]).filtered) == 2113665
    check_files(codec, files)


def test_huffman_only_and_rle(codec):
    a = C.rgb_image(64, 64)
    check_files(codec, [M.make_png(a, 4, level=9, strategy=zlib.Z_HUFFMAN_ONLY), M.make_png(a, 4, level=9, strategy=zlib.Z_RLE)])


@pytest.fixture(scope="module")
def recons():
    with np.load(os.path.join(GOLDEN, "imagenet4_trained.npz")) as g:
        small = g["recon"]
    with np.load(os.path.join(GOLDEN, "kodim21_256_trained.npz")) as g:
        big, latent = g["recon"], g["latent"]
    return small, big, latent


def test_round_trip_of_every_writer(codec, recons):
    import torch

    from neural_network_image_compression_amd import bitstream as B

    for x in recons[:2]:
        want = torch.from_numpy(x).cuda()
        sets = [[C.pillow_png(a, optimize=True) for a in x], B.png_encode(x, mode="pillow"), B.png_encode(x, mode="tf"),
                B.png_files_device(codec, want, "adaptive"), B.png_files_device(codec, want, 4)]
        for files in sets:
            assert torch.equal(check_files(codec, files), want)
    assert sum(b["type"] == "dynamic" for b in png_parse.deflate_blocks(png_parse.parse(sets[0][0]).idat)) >= 2


def test_packed_latent_png_unpacks_to_the_golden_latent(codec, recons):
    import torch

    latent = torch.from_numpy(recons[2]).cuda()
    packed = codec.pack(latent)
    assert tuple(packed.shape) == (1, 128, 256, 3)
    images = check_files(codec, [C.pillow_png(packed[0].cpu().numpy(), optimize=True)])
    assert torch.equal(codec.unpack(images), latent)


def test_batch_invariance_across_stream_lengths(codec):
    import torch

    flat = np.full((64, 64, 3), 9, np.uint8)
    noise = np.random.default_rng(0).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    files = [C.pillow_png(flat, optimize=True), C.pillow_png(noise, optimize=True)]
    assert len(png_parse.parse(files[1]).idat) > 100 * len(png_parse.parse(files[0]).idat)  # 12,363 against 78 bytes
    both = check_files(codec, files)
    for i in range(2):
        assert torch.equal(check_files(codec, [files[i]])[0], both[i])


@pytest.mark.parametrize("name", sorted(C.status_streams()))
def test_status_bits(codec, name):
    import torch

    bad, T, bits = C.status_streams()[name]
    h, w = C.STATUS_SHAPE
    a = C.rgb_image(h, w)
    good, T2 = C.stream_of(a, 2, level=9)
    assert T == T2
    images, status = read_streams(codec, [good, bad, good], h, w, 3)
    assert status.cpu().tolist() == [0, bits, 0]
    want = torch.from_numpy(a).to(images.device)
    assert torch.equal(images[0], want) and torch.equal(images[2], want)
    with pytest.raises(ValueError, match="image 1"):
        from neural_network_image_compression_amd import bitstream as B

        codec.png_read(*B._upload_files(codec, [good, bad]), h, w, 3)


def test_read_png_device_groups_and_falls_back(codec):
    import torch

    from neural_network_image_compression_amd import bitstream as B

    a, b = C.rgb_image(8, 8), C.rgb_image(37, 53)
    files = [C.pillow_png(a), C.pillow_png(b), C.interlaced_png(a), M.make_png(a, 3)]
    groups = B.read_png_device(codec, files)
    assert [idx for idx, _ in groups] == [[0, 2, 3], [1]]
    for idx, t in groups:
        assert torch.equal(t.cpu(), torch.from_numpy(np.stack([pillow_pixels(files[i]) for i in idx])))
    with pytest.raises(ValueError, match="file 1"):
        B.read_png_device(codec, [files[0], C.corrupt_files()["flipped_crc"]])


def _dir_bytes(path):
    return {fn: open(os.path.join(path, fn), "rb").read() for fn in sorted(os.listdir(path))}


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory, weights_trained):
    from neural_network_image_compression_amd import weights as W

    d = tmp_path_factory.mktemp("ck")
    W.save(weights_trained, str(d / "encoder"), "encoder")
    W.save(weights_trained, str(d / "decoder"), "decoder")
    return d


def test_compress_with_the_device_reader_writes_the_same_files(codec, ckpt, tmp_path):
    from neural_network_image_compression_amd.codec import Encoder

    a, b = C.rgb_image(64, 64), C.rgb_image(37, 53)
    outs = {}
    for reader in ("pillow", "device"):
        d = tmp_path / reader
        d.mkdir()
        Image.fromarray(a).save(d / "a.jpg", quality=90)
        (d / "b.png").write_bytes(C.pillow_png(a, optimize=True))
        (d / "c.png").write_bytes(C.pillow_png(b, optimize=True))
        (d / "d.png").write_bytes(C.interlaced_png(a[::-1].copy()))
        (d / "e.png").write_bytes(M.make_png(a[:, ::-1].copy(), 4, level=9))
        Image.fromarray(a[::2].repeat(2, 0)).save(d / "f.jpg", quality=90)
        Encoder(codec=codec).compress(str(d), str(ckpt / "encoder"), container="nic", png_reader=reader)
        outs[reader] = _dir_bytes(str(d) + "_compressed")
    assert sorted(outs["pillow"]) == ["a.nic", "b.nic", "c.nic", "d.nic", "e.nic", "f.nic"]
    assert outs["device"] == outs["pillow"]


def test_uncompress_with_the_device_reader_writes_the_same_files(codec, ckpt, tmp_path):
    import torch

    from neural_network_image_compression_amd.codec import Decoder

    packed = []
    for name in ("imagenet4_trained", "kodim21_256_trained"):  # four 64x128 packed latents and a 128x256 one
        with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
            packed += list(codec.pack(torch.from_numpy(g["latent"]).cuda()).cpu().numpy())
    outs = {}
    for reader in ("pillow", "device"):
        d = tmp_path / reader / "tiles_compressed"
        d.mkdir(parents=True)
        for i, p in enumerate(packed):
            (d / f"t{i}.png").write_bytes(C.pillow_png(p, optimize=True))
        Decoder(codec=codec).uncompress(str(d), str(ckpt / "decoder"), container="png", png_reader=reader, png_writer="device")
        outs[reader] = _dir_bytes(str(d).replace("compressed", "uncompressed"))
    assert len(outs["pillow"]) == len(packed)
    assert outs["device"] == outs["pillow"]
