"""Batched region decode on the device (csrc/nic_rans.hip: the per-file-window form of rans_parse and
rans_decode_segments, cut_boxes; bitstream.decode_regions): one call over files of different frame
sizes gives the crops of the whole reconstructions, in the files' order, for every container version
and both precision modes; the window decode and the cut store nothing outside their outputs; a
status belongs to its file alone; a table row that does not fit its file is refused on the device."""
import numpy as np
import pytest

from tests import rans2_ref as R2
from tests import rans3_ref as R3
from tests import rans_ref as R
from tests.test_region_batch_format import BOX, LATENTS, boxes_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import bitstream as B  # noqa: E402
from neural_network_image_compression_amd.codec import Codec, Decoder  # noqa: E402
from neural_network_image_compression_amd.prior import ContextPrior, Prior  # noqa: E402

VERSIONS = (1, 2, 3)
SHAPE = (12, 10)  # the fixed window of a 40 x 24 box; the 20x9 latent is narrower: (12, 9)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def latents(golden):
    """Four parts of kodim21_full's spread-weight latent (64x96), of test_region_batch_format's shapes."""
    zf = golden("kodim21_full")["latent"][0]
    corner = {(13, 15): (0, 0), (20, 9): (10, 40), (40, 70): (0, 0), (32, 32): (30, 60)}
    return [np.ascontiguousarray(zf[r:r + h8, c:c + w8]) for (h8, w8), (r, c) in ((s, corner[s]) for s in LATENTS)]


@pytest.fixture(scope="module")
def codec(latents):
    """A codec without weights (the coder needs none) and the two priors, fitted on the 40x70 latent."""
    c = Codec(0)
    static = Prior.accumulator(c).add(_dev(latents[2][None])).build()
    cprior = ContextPrior.accumulator(c, static).add(_dev(latents[2][None])).build()
    yield c, static, cprior
    c.close()


def _set_version(c, static, cprior, ver):
    """nic_files writes version 3 under a context prior, else version 2 under a prior, else version 1."""
    c.set_prior(static if ver == 2 else None)
    c.set_context_prior(cprior if ver == 3 else None)


def _files(c, latents, ver, seg_pixels=B.NIC_SEG_PIXELS):
    files = [B.nic_files(c, _dev(z[None]), seg_pixels)[0] for z in latents]
    assert all(f[4] == ver for f in files)
    return files


def _table(latents, boxes):
    """(h8, w8, r0, c0) per file and its window shape, from region_plan_fixed."""
    rows = []
    for z, box in zip(latents, boxes):
        h8, w8 = z.shape[:2]
        (r0, c0, nr, nc), _ = Codec.region_plan_fixed(8 * h8, 8 * w8, box)
        rows.append(((h8, w8, r0, c0), (nr, nc)))
    return rows


def _windows_status(c, ver):
    return {1: c.rans_decode_windows_status, 2: c.rans2_decode_windows_status, 3: c.rans3_decode_windows_status}[ver]


# ---- end to end -----------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("ver", VERSIONS)
def test_decode_regions_is_the_crop_of_every_whole_decode(codec, latents, weights_spread, ver, precision):
    """Every file at the four corners, an edge and the interior, position-major, so the 20x9 file's
    group (12, 9) alternates with the others' (12, 10) in the input: 24 boxes, one call."""
    _, static, cprior = codec
    dec = Decoder(0, precision=precision)
    try:
        dec.set_weights(weights_spread)
        _set_version(dec.codec, static, cprior, ver)
        files = _files(dec.codec, latents, ver)
        wholes = [dec.codec.decode(_dev(z[None]))[0] for z in latents]
        order = [(i, boxes_of(*latents[i].shape[:2])[k]) for k in range(6) for i in range(len(latents))]
        shapes = [Codec.region_plan_fixed(8 * latents[i].shape[0], 8 * latents[i].shape[1], box)[0][2:] for i, box in order]
        assert set(shapes) == {SHAPE, (12, 9)} and shapes[:4] == [SHAPE, (12, 9), SHAPE, SHAPE]
        got = dec.decode_regions([files[i] for i, _ in order], [box for _, box in order])
        assert tuple(got.shape) == (24, BOX[0], BOX[1], 3) and got.is_contiguous() and got.dtype == torch.uint8
        for n, (i, (y, x, h, w)) in enumerate(order):
            ref = wholes[i][y:y + h, x:x + w]
            single = dec.decode_region([files[i]], (y, x, h, w))[0]
            diff, diff1 = int((got[n] != ref).sum()), int((got[n] != single).sum())
            print(f"v{ver} {precision} latent {latents[i].shape[:2]} box {(y, x, h, w)}: {diff} differing bytes from the whole "
                  f"decode, {diff1} from decode_region")
            assert torch.equal(got[n], ref) and torch.equal(got[n], single), (i, y, x)
        # one group: the files' order without a gather
        same = [0, 2, 3, 2]
        got = dec.decode_regions([files[i] for i in same], [boxes_of(*latents[i].shape[:2])[5] for i in same])
        for n, i in enumerate(same):
            y, x, h, w = boxes_of(*latents[i].shape[:2])[5]
            assert torch.equal(got[n], wholes[i][y:y + h, x:x + w])
        assert tuple(dec.decode_regions([], []).shape) == (0, 0, 0, 3)
    finally:
        dec.codec.close()


def test_python_checks(codec, latents, tmp_path):
    c, static, cprior = codec
    _set_version(c, static, cprior, 1)
    files = _files(c, latents, 1)
    dec = Decoder(codec=c)
    (tmp_path / "narrow.nic").write_bytes(files[1])
    ok = [boxes_of(*z.shape[:2])[0] for z in latents]
    with pytest.raises(ValueError, match="file 2.*share one size"):
        dec.decode_regions(files, ok[:2] + [(0, 0, 40, 25)] + ok[3:])
    with pytest.raises(ValueError, match="3 boxes for 4 files"):
        dec.decode_regions(files, ok[:3])
    with pytest.raises(ValueError, match=r"narrow\.nic.*does not lie inside its 160 x 72 image"):
        dec.decode_regions([files[0], str(tmp_path / "narrow.nic")], [ok[0], (0, 49, 40, 24)])
    with pytest.raises(ValueError, match="file 1.*does not lie inside"):
        B.read_nic_windows(c, files[:2], [ok[0], (121, 0, 40, 24)])
    _set_version(c, static, cprior, 2)
    files2 = _files(c, latents[:1], 2)
    with pytest.raises(ValueError, match="file 1.*version 2.*version 1"):
        dec.decode_regions([files[0], files2[0]], ok[:2])
    # the groups of read_nic_windows: indices, window latents, offsets
    _set_version(c, static, cprior, 1)
    groups = B.read_nic_windows(c, files, [boxes_of(*z.shape[:2])[3] for z in latents])
    assert [g[0] for g in groups] == [[0, 2, 3], [1]]
    for idx, z, offs in groups:
        for n, i in enumerate(idx):
            h8, w8 = latents[i].shape[:2]
            (r0, c0, nr, nc), off = Codec.region_plan_fixed(8 * h8, 8 * w8, boxes_of(h8, w8)[3])
            assert offs[n] == off and tuple(z.shape[1:]) == (nr, nc, 96)
            np.testing.assert_array_equal(z[n].cpu().numpy(), latents[i][r0:r0 + nr, c0:c0 + nc])


# ---- the window entropy decode ------------------------------------------------------------------

@pytest.mark.parametrize("ver", VERSIONS)
def test_no_store_outside_the_output(codec, latents, ver):
    """Segments of 7, 32 and 100 pixels; the three files of window shape (12, 10), each at another position."""
    c, static, cprior = codec
    _set_version(c, static, cprior, ver)
    keep = [0, 2, 3]
    zs = [latents[i] for i in keep]
    for S, k in ((7, 5), (32, 3), (100, 1)):
        plan = _table(zs, [boxes_of(*z.shape[:2])[(k + j) % 6] for j, z in enumerate(zs)])
        assert all(shape == SHAPE for _, shape in plan)
        buf, sizes = B._upload_files(c, _files(c, zs, ver, S))
        count, pad = 3 * SHAPE[0] * SHAPE[1] * 96, 4096
        big = torch.full((pad + count + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[pad:pad + count].view(3, *SHAPE, 96)
        got, status = _windows_status(c, ver)(buf, sizes, [row for row, _ in plan], SHAPE, out=out)
        assert got.data_ptr() == out.data_ptr() and status.cpu().tolist() == [0, 0, 0]
        for n, ((h8, w8, r0, c0), _) in enumerate(plan):
            np.testing.assert_array_equal(out[n].cpu().numpy(), zs[n][r0:r0 + SHAPE[0], c0:c0 + SHAPE[1]], str((S, n)))
        assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + count:] == 0xA5).all())
        # the table on the device, with the bound it then needs
        tab = torch.tensor([row for row, _ in plan], dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match="max_pixels"):
            _windows_status(c, ver)(buf, sizes, tab, SHAPE)
        again, status = _windows_status(c, ver)(buf, sizes, tab, SHAPE, max_pixels=40 * 70)
        assert status.cpu().tolist() == [0, 0, 0] and torch.equal(again, out)


@pytest.mark.parametrize("ver", VERSIONS)
def test_status_is_per_file(codec, latents, ver):
    c, static, cprior = codec
    _set_version(c, static, cprior, ver)
    keep = [0, 2, 3]
    zs = [latents[i] for i in keep]
    plan = _table(zs, [boxes_of(*z.shape[:2])[5] for z in zs])
    table = [row for row, _ in plan]
    files = _files(c, zs, ver)
    want = [z[r0:r0 + SHAPE[0], c0:c0 + SHAPE[1]] for z, (_, _, r0, c0) in zip(zs, table)]
    parse = {1: R.parse_file, 2: R2.parse_file, 3: R3.parse_file}[ver]

    def run(datas, lens=None, tab=table, **more):
        buf, sizes = B._upload_files(c, datas)
        if lens is not None:
            sizes = torch.tensor(lens, dtype=torch.int64, device="cuda")
        out = torch.full((3, *SHAPE, 96), 0xA5, dtype=torch.uint8, device="cuda")
        _, status = _windows_status(c, ver)(buf, sizes, tab, SHAPE, out=out, **more)
        return out.cpu().numpy(), status.cpu().tolist()

    def others_intact(out, bad):
        for n in range(3):
            if n != bad:
                np.testing.assert_array_equal(out[n], want[n])

    out, status = run(files)
    assert status == [0, 0, 0]
    others_intact(out, None)
    # a payload byte flipped in the segment that holds the first pixel of file 1's window: a decode error
    info = parse(files[1])
    _, w8, r0, c0 = table[1]
    k = (r0 * w8 + c0) // B.NIC_SEG_PIXELS
    d = bytearray(files[1])
    d[info["payload"] + sum(info["seg_lengths"][:k]) + info["seg_lengths"][k] // 2] ^= 0x5A
    out, status = run([files[0], bytes(d), files[2]])
    assert status == [0, 1, 0]
    others_intact(out, 1)
    # ... and in a segment below the window: not decoded, not seen
    k = ((r0 + SHAPE[0]) * w8 + w8) // B.NIC_SEG_PIXELS + 1
    d = bytearray(files[1])
    d[info["payload"] + sum(info["seg_lengths"][:k]) + info["seg_lengths"][k] // 2] ^= 0x5A
    out, status = run([files[0], bytes(d), files[2]])
    assert status == [0, 0, 0]
    others_intact(out, None)
    # file 2 cut off inside its header: only its header bit, and nothing of it is written
    out, status = run(files, lens=[len(files[0]), len(files[1]), 12])
    assert status == [0, 0, 2]
    others_intact(out, 2)
    assert (out[2] == 0xA5).all()
    decode = {1: c.rans_decode_windows, 2: c.rans2_decode_windows, 3: c.rans3_decode_windows}[ver]
    buf, sizes = B._upload_files(c, [files[0], bytes(d[:20]), files[2]])
    with pytest.raises(ValueError, match="image 1 is corrupt"):
        decode(buf, sizes, table, SHAPE)
    # table rows that do not fit their file: each is refused alone, on the device
    h8, w8, r0, c0 = table[1]
    for row in ((h8, w8, h8 - SHAPE[0] + 1, c0), (h8, w8, r0, w8 - SHAPE[1] + 1), (h8, w8, -1, c0), (h8, w8, r0, -1),
                (h8 + 1, w8, r0, c0), (w8, h8, r0, c0), (0, w8, 0, 0), (-h8, -w8, r0, c0), (2 ** 31 - 1, 2 ** 31 - 1, r0, c0),
                (h8, w8, 2 ** 31 - 1, c0)):
        out, status = run(files, tab=[table[0], row, table[2]])
        assert status == [0, 2, 0], row
        others_intact(out, 1)
        assert (out[1] == 0xA5).all(), row
    # a file larger than the caller's bound is refused, not indexed
    tab = torch.tensor(table, dtype=torch.int32, device="cuda")
    out, status = run(files, tab=tab, max_pixels=32 * 32)
    assert status == [0, 2, 0]
    others_intact(out, 1)
    assert (out[1] == 0xA5).all()


# ---- the cut ----------------------------------------------------------------------------------------

def test_cut_boxes(codec):
    c = codec[0]
    rng = np.random.default_rng(5)
    for n, Hs, Ws, h, w in ((3, 96, 80, 40, 24), (5, 17, 23, 5, 7), (2, 9, 9, 9, 9), (1, 64, 64, 1, 1), (300, 40, 33, 31, 29)):
        x = rng.integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)
        offs = np.stack([rng.integers(0, Hs - h + 1, n), rng.integers(0, Ws - w + 1, n)], axis=1)
        offs[0] = (Hs - h, Ws - w)
        count, pad = n * h * w * 3, 1024
        big = torch.full((pad + count + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[pad:pad + count].view(n, h, w, 3)
        got = c.cut_boxes(_dev(x), offs.tolist(), h, w, out=out)
        assert got.data_ptr() == out.data_ptr()
        want = np.stack([x[i, oy:oy + h, ox:ox + w] for i, (oy, ox) in enumerate(offs.tolist())])
        np.testing.assert_array_equal(out.cpu().numpy(), want, str((n, Hs, Ws, h, w)))
        assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + count:] == 0xA5).all())
        # the table on the device gives the same
        assert torch.equal(c.cut_boxes(_dev(x), torch.tensor(offs, dtype=torch.int32, device="cuda"), h, w), out)
    x = _dev(rng.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8))
    for bad in ([(0, 0), (9, 0)], [(0, 9), (0, 0)], [(-1, 0), (0, 0)], [(0, 0), (0, -1)]):
        with pytest.raises(ValueError, match=f"image {0 if bad[0] != (0, 0) else 1}"):
            c.cut_boxes(x, bad, 8, 8)
    with pytest.raises(ValueError):
        c.cut_boxes(x, [(0, 0)], 8, 8)
    with pytest.raises(ValueError):
        c.cut_boxes(x, [(0, 0), (0, 0)], 17, 8)
    # unchecked offsets on the device: what lies outside the image reads as 0, nothing else is touched
    got = c.cut_boxes(x, torch.tensor([[12, -3], [0, 0]], dtype=torch.int32, device="cuda"), 8, 8).cpu().numpy()
    want = np.zeros((8, 8, 3), np.uint8)
    want[:4, 3:] = x[0, 12:16, 0:5].cpu().numpy()
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], x[1, :8, :8].cpu().numpy())
