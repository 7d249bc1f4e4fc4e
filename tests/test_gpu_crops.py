"""Crops of mixed sizes on the device (csrc/nic_resample.hip: resample_boxes; bitstream.decode_crops):
the resample kernel against tests/resample_ref.py for every output kind, with flips, a scattered dst
and nothing stored outside its rows; bit-for-bit identity at equal sizes; a device table the host did
not check; Decoder.decode_crops over files of different frame sizes and boxes of five sizes against
the resampled crop of every whole decode, for every container version and both precision modes.

The tolerance is derived, not measured (resample_ref.crop): every fp32 operation errs by at most 2^-24
relative on partial sums of at most 255, so a float output may differ from the float64 reference by
(4 + Ty + Tx) 2^-23 / std_c + 2^-23 |ref|, Ty and Tx that output's tap counts (the factor 2 over the
sum of the roundings is the margin); f16 adds 2^-11 |ref|; u8 is within 0.5 plus the same bound, in
0..255 units, of the reference before its rounding."""
import numpy as np
import pytest

from tests import resample_ref as RR
from tests.test_gpu_region_batch import _dev, _files, _set_version, codec, latents  # noqa: F401  (fixtures)
from tests.test_region_batch_format import LATENTS, boxes_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import bitstream as B  # noqa: E402
from neural_network_image_compression_amd.codec import Decoder  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KINDS = {"float32": torch.float32, "float16": torch.float16, "uint8": torch.uint8}
SENTINEL = {"float32": -777.0, "float16": -777.0, "uint8": 0xA5}
HS, WS = 96, 80
# (oy, ox, bh, bw, flip): 40x24, 17x33, 1x1, 9x9 and the whole image, flips on and off; two rows per call
ROWS = [(3, 50, 40, 24, 0), (79, 47, 17, 33, 1), (95, 0, 1, 1, 1), (0, 71, 9, 9, 0), (0, 0, HS, WS, 1), (56, 0, 40, 24, 1)]
DST = [5, 2, 7, 0, 3, 6]  # into n_out = 8: images 1 and 4 stay untouched
N_OUT = 8


@pytest.fixture(scope="module")
def images():
    return np.random.default_rng(21).integers(0, 256, (2, HS, WS, 3), dtype=np.uint8)


def _framed(n_out, size, kind, pad=256):
    """out (n_out, ...) of one kind inside a larger allocation, everything filled with the kind's sentinel."""
    shape = (n_out, *size, 3) if kind == "uint8" else (n_out, 3, *size)
    count = int(np.prod(shape))
    big = torch.full((pad + count + pad,), SENTINEL[kind], dtype=KINDS[kind], device="cuda")
    return big, big[pad:pad + count].view(shape), pad, count


def _check(got, image, row, size, kind, what):
    ref, tol = RR.crop(image, row, size, kind, MEAN, STD)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: max |got - ref| {err.max():.3e}, max of the bound's use {(err / tol).max():.3f}")
    assert got.shape == ref.shape and (err <= tol).all(), what


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("size", [(16, 16), (7, 5), (32, 24)])
def test_resample_boxes_is_the_restatement(codec, images, size, kind):
    c = codec[0]
    x = _dev(images)
    big, out, pad, count = _framed(N_OUT, size, kind)
    for k in range(0, len(ROWS), 2):
        table = [(*ROWS[k + j], DST[k + j]) for j in range(2)]
        # the table from the host, and for the last pair from the device
        tab = table if k < 4 else torch.tensor(table, dtype=torch.int32, device="cuda")
        got = c.resample_boxes(x, tab, size, KINDS[kind], MEAN, STD, out=out)
        assert got.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    for k, (row, dst) in enumerate(zip(ROWS, DST)):
        _check(host[dst], images[k % 2], row, size, kind, f"{kind} {row} -> {size}")
    sentinel = SENTINEL[kind]
    assert bool((out[1] == sentinel).all()) and bool((out[4] == sentinel).all())
    assert bool((big[:pad] == sentinel).all()) and bool((big[pad + count:] == sentinel).all())
    # a new tensor of n_out = N when none is given
    got = c.resample_boxes(x, [(*ROWS[0], 1), (*ROWS[1], 0)], size, KINDS[kind], MEAN, STD)
    assert got.dtype == KINDS[kind] and got.shape[0] == 2 and got.is_contiguous()
    assert torch.equal(got[1], out[DST[0]]) and torch.equal(got[0], out[DST[1]])


def test_a_scale_too_large_to_stage_reads_global_memory(codec):
    """768 x 1024 -> 32 x 32: a tile's source rows are far above the LDS budget and the tap counts (49 and
    65) above any fixed table; and 300 x 420 -> 224 x 224, more than one tile per axis, staged."""
    c = codec[0]
    rng = np.random.default_rng(22)
    for (Hs, Ws), size, row in (((768, 1024), (32, 32), (0, 0, 768, 1024, 1)), ((300, 420), (224, 224), (7, 9, 290, 405, 0))):
        image = rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)
        for kind in ("float32", "uint8"):
            big, out, pad, count = _framed(1, size, kind)
            c.resample_boxes(_dev(image), [(*row, 0)], size, KINDS[kind], MEAN, STD, out=out)
            _check(out[0].cpu().numpy(), image[0], row, size, kind, f"{kind} {row} -> {size}")
            assert bool((big[:pad] == SENTINEL[kind]).all()) and bool((big[pad + count:] == SENTINEL[kind]).all())


def test_equal_sizes_give_the_source_pixels(codec, images):
    c = codec[0]
    x = _dev(images)
    for (bh, bw), offs in (((40, 24), [(3, 50), (56, 0)]), ((17, 33), [(79, 47), (0, 1)]), ((HS, WS), [(0, 0), (0, 0)])):
        table = [(oy, ox, bh, bw, 0, i) for i, (oy, ox) in enumerate(offs)]
        got = c.resample_boxes(x, table, (bh, bw), torch.uint8)
        assert torch.equal(got, c.cut_boxes(x, offs, bh, bw)), (bh, bw)
        # and mirrored, and as floats: v / 255 in one fma from the pixel itself
        table = [(oy, ox, bh, bw, 1, i) for i, (oy, ox) in enumerate(offs)]
        assert torch.equal(c.resample_boxes(x, table, (bh, bw), torch.uint8), got.flip(2))
        f = c.resample_boxes(x, table, (bh, bw), torch.float32)
        want = got.flip(2).permute(0, 3, 1, 2).to(torch.float32) * np.float32(1.0 / 255.0)
        assert torch.equal(f, want)


def test_a_table_the_host_did_not_check(codec, images):
    """Rows the kernel is specified to refuse, in a device table that no host code read: each leaves
    every sentinel of out intact and the good row beside it is correct."""
    c = codec[0]
    x = _dev(images)
    size, kind = (7, 5), "float32"
    good = (3, 50, 40, 24, 1)
    big_int = 2 ** 31 - 1
    bad_rows = [(-1, 0, 8, 8, 0, 0), (0, -1, 8, 8, 0, 0), (HS - 7, 0, 8, 8, 0, 0), (0, WS - 7, 8, 8, 0, 0), (0, 0, HS + 1, 8, 0, 0),
                (0, 0, 0, 8, 0, 0), (0, 0, 8, 0, 0, 0), (0, 0, -8, 8, 0, 0), (0, 0, 8, 8, 7, 0), (0, 0, 8, 8, -1, 0),
                (0, 0, 8, 8, 0, -1), (0, 0, 8, 8, 0, 3), (big_int, 0, 8, 8, 0, 0), (1, 0, big_int, 8, 0, 0), (0, 1, 8, big_int, 0, 0),
                (0, 0, 8, 8, 0, big_int), (-big_int, -big_int, big_int, big_int, 0, 0)]
    ref, tol = RR.crop(images[1], good, size, kind, MEAN, STD)
    for bad in bad_rows:
        big, out, pad, count = _framed(3, size, kind)
        table = torch.tensor([bad, (*good, 2)], dtype=torch.int32, device="cuda")
        c.resample_boxes(x, table, size, KINDS[kind], MEAN, STD, out=out)
        host = out.cpu().numpy()
        assert (host[:2] == SENTINEL[kind]).all(), bad
        assert (np.abs(host[2] - ref) <= tol).all(), bad
        assert bool((big[:pad] == SENTINEL[kind]).all()) and bool((big[pad + count:] == SENTINEL[kind]).all()), bad
    torch.cuda.synchronize()
    # the same rows from the host are refused before the upload, by their row
    for bad in bad_rows[:12]:
        with pytest.raises(ValueError, match="row 1"):
            c.resample_boxes(x, [(*good, 2), bad], size, KINDS[kind], MEAN, STD, n_out=3)
    with pytest.raises(ValueError, match="3 table rows for 2 images"):
        c.resample_boxes(x, [(*good, 0)] * 3, size)
    with pytest.raises(ValueError, match="dtype"):
        c.resample_boxes(x, [(*good, 0)] * 2, size, torch.int32)
    with pytest.raises(ValueError, match="std"):
        c.resample_boxes(x, [(*good, 0)] * 2, size, std=(1, 0, 1))
    with pytest.raises(ValueError):
        c.resample_boxes(x, [(*good, 0)] * 2, (0, 5))


# ---- end to end ---------------------------------------------------------------------------------

SIZE = (16, 12)
BOX_SIZES = ((40, 24), (9, 17), (64, 56), (96, 33))  # and the whole 160 x 72 image of the 20x9 latent


def _order():
    """24 boxes: the four files at boxes_of's six positions, the box sizes rotating; one box of the 20x9
    file is its whole image."""
    order = []
    for k in range(6):
        for i, (h8, w8) in enumerate(LATENTS):
            bh, bw = BOX_SIZES[(k + i) % 4]
            order.append((i, boxes_of(h8, w8, bh, bw)[k]))
    order[9] = (1, (0, 0, 160, 72))
    assert LATENTS[order[9][0]] == (20, 9) and len({b[2:] for _, b in order}) == 5
    return order


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("ver", (1, 2, 3))
def test_decode_crops_is_the_resampled_crop_of_every_whole_decode(codec, latents, weights_spread, ver, precision):
    _, static, cprior = codec
    dec = Decoder(0, precision=precision)
    try:
        dec.set_weights(weights_spread)
        _set_version(dec.codec, static, cprior, ver)
        files = _files(dec.codec, latents, ver)
        wholes = [dec.codec.decode(_dev(z[None]))[0].cpu().numpy() for z in latents]
        order = _order()
        flips = [n % 2 == 1 for n in range(12)] + [n % 3 == 0 for n in range(12)]
        names, boxes = [files[i] for i, _ in order], [b for _, b in order]
        groups = B.read_nic_windows_any(dec.codec, names, boxes)
        assert [tuple(z.shape[1:3]) for _, z, _ in groups] == [(13, 15), (20, 9), (27, 16)]  # the one target, clamped to the two smaller latents
        assert sorted(i for idx, _, _ in groups for i in idx) == list(range(24))
        assert len(B.read_nic_windows_any(dec.codec, names, boxes, bucket=8)) > 3
        got = dec.decode_crops(names, boxes, SIZE, flip=flips, mean=MEAN, std=STD)
        assert tuple(got.shape) == (24, 3, *SIZE) and got.dtype == torch.float32 and got.is_contiguous()
        host = got.cpu().numpy()
        for n, (i, box) in enumerate(order):
            _check(host[n], wholes[i], (*box, flips[n]), SIZE, "float32", f"v{ver} {precision} latent {LATENTS[i]} box {box}")
        # the pixels under the resampler do not depend on the window: other groups, the same tensor
        assert torch.equal(dec.decode_crops(names, boxes, SIZE, flip=flips, mean=MEAN, std=STD, bucket=8), got)
        if ver == 1 and precision == "fp32":
            half = dec.decode_crops(names, boxes, SIZE, flip=flips, mean=MEAN, std=STD, dtype=torch.float16)
            assert half.dtype == torch.float16 and torch.equal(half, got.to(torch.float16))
            u8 = dec.decode_crops(names[:5], boxes[:5], SIZE, dtype=torch.uint8)
            assert tuple(u8.shape) == (5, *SIZE, 3) and u8.dtype == torch.uint8
            for n, (i, box) in enumerate(order[:5]):
                _check(u8[n].cpu().numpy(), wholes[i], (*box, 0), SIZE, "uint8", f"u8 latent {LATENTS[i]} box {box}")
            assert tuple(dec.decode_crops([], [], SIZE).shape) == (0, 3, *SIZE)
            assert tuple(dec.decode_crops([], [], SIZE, dtype=torch.uint8).shape) == (0, *SIZE, 3)
    finally:
        dec.codec.close()


def test_python_checks(codec, latents, tmp_path):
    c, static, cprior = codec
    _set_version(c, static, cprior, 1)
    files = _files(c, latents, 1)
    dec = Decoder(codec=c)
    (tmp_path / "narrow.nic").write_bytes(files[1])
    ok = [boxes_of(h8, w8, *BOX_SIZES[i])[0] for i, (h8, w8) in enumerate(LATENTS)]
    with pytest.raises(ValueError, match=r"narrow\.nic.*does not lie inside its 160 x 72 image"):
        dec.decode_crops([files[0], str(tmp_path / "narrow.nic")], [ok[0], (0, 49, 40, 24)], SIZE)
    with pytest.raises(ValueError, match="file 2.*does not lie inside"):
        dec.decode_crops(files, ok[:2] + [(0, 0, 321, 8)] + ok[3:], SIZE)
    with pytest.raises(ValueError, match="3 boxes for 4 files"):
        dec.decode_crops(files, ok[:3], SIZE)
    with pytest.raises(ValueError, match="3 flips for 4 files"):
        dec.decode_crops(files, ok, SIZE, flip=[0, 1, 0])
    for size in ((0, 12), (16, 16385), (16,), 16):
        with pytest.raises(ValueError, match="size"):
            dec.decode_crops(files, ok, size)
    with pytest.raises(ValueError, match="std"):
        dec.decode_crops(files, ok, SIZE, std=(0.2, 0.0, 0.2))
    with pytest.raises(ValueError, match="dtype"):
        dec.decode_crops(files, ok, SIZE, dtype=torch.int32)
    for bucket in (0, -8, 2.5):
        with pytest.raises(ValueError, match="bucket"):
            dec.decode_crops(files, ok, SIZE, bucket=bucket)
    _set_version(c, static, cprior, 2)
    files2 = _files(c, latents[:1], 2)
    with pytest.raises(ValueError, match="file 1.*version 2.*version 1"):
        dec.decode_crops([files[0], files2[0]], ok[:2], SIZE)
    _set_version(c, static, cprior, 1)
    # decode_regions keeps its rule: boxes of one size
    with pytest.raises(ValueError, match="file 1.*share one size"):
        dec.decode_regions(files, ok)
    with pytest.raises(ValueError, match="file 1.*share one size"):
        B.read_nic_windows(c, files, ok)
