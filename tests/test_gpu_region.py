"""Region decode on the device (csrc/nic_rans.hip: rans_decode_window_segments and
rans3_decode_window_segments; bitstream.decode_region and the directory drivers): the window entropy
decode is the slice of the full one for every container version, it stores nothing outside its
output, its statuses cover what it decoded, decode_region is the crop of the whole reconstruction in
both precision modes, and uncompress(region=...) writes those crops."""
import os

import numpy as np
import pytest

from tests import rans2_ref as R2
from tests import rans3_ref as R3
from tests import rans_ref as R
from tests.test_region_format import LATENTS, SEG_PIXELS, segments, windows_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import _lib  # noqa: E402
from neural_network_image_compression_amd import bitstream as B  # noqa: E402
from neural_network_image_compression_amd.codec import Codec, Decoder, Encoder  # noqa: E402
from neural_network_image_compression_amd.prior import ContextPrior, Prior  # noqa: E402

VERSIONS = (1, 2, 3)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def codec():
    c = Codec(0)  # the coder needs no weights
    yield c
    c.set_prior(None)
    c.set_context_prior(None)
    c.close()


@pytest.fixture(scope="module")
def latents():
    """Seeded skewed latents of test_region_format's shapes; 13x15 is a batch of 3 different ones."""
    rng = np.random.default_rng(23)
    return {(h8, w8): np.minimum(rng.geometric(0.3, (3 if (h8, w8) == (13, 15) else 1, h8, w8, 96)) - 1, 255).astype(np.uint8)
            for h8, w8 in LATENTS}


@pytest.fixture(scope="module")
def priors(latents):
    """Fitted as in tests/test_gpu_rans3.py, on the 13x15 batch: (static freqs, (anchors, context freqs))."""
    return R2.fit_prior(latents[(13, 15)]), R3.fit_context_prior(latents[(13, 15)])


def _use(codec, priors, ver):
    """The codec's priors for files of version ver, and (encode, decode_status, window_status, reference reader)."""
    codec.set_prior(Prior(priors[0]) if ver == 2 else None)
    codec.set_context_prior(ContextPrior(*priors[1]) if ver == 3 else None)
    return {1: (codec.rans_encode, codec.rans_decode_status, codec.rans_decode_window_status, R.read_file),
            2: (codec.rans2_encode, codec.rans2_decode_status, codec.rans2_decode_window_status,
                lambda d: R2.read_file(d, priors[0])),
            3: (codec.rans3_encode, codec.rans3_decode_status, codec.rans3_decode_window_status,
                lambda d: R3.read_file(d, priors[1]))}[ver]


def _check_windows(z, seg_pixels, calls, wins, reference=True):
    encode, decode_status, window_status, read_ref = calls
    n, h8, w8, _ = z.shape
    buf, sizes = encode(_dev(z), seg_pixels)
    full, status = decode_status(buf, sizes, h8, w8)
    assert status.cpu().tolist() == [0] * n
    full_h = full.cpu().numpy()
    np.testing.assert_array_equal(full_h, z)
    if reference:  # the CPU reference coder reads the device's files to the same latents
        host, sizes_h = buf.cpu().numpy(), sizes.cpu().numpy()
        for i in range(n):
            np.testing.assert_array_equal(read_ref(host[i, :sizes_h[i]].tobytes()), full_h[i])
    for win in wins:
        r0, c0, rows, cols = win
        got, status = window_status(buf, sizes, h8, w8, win)
        assert status.cpu().tolist() == [0] * n, (seg_pixels, win)
        assert tuple(got.shape) == (n, rows, cols, 96)
        assert torch.equal(got, full[:, r0:r0 + rows, c0:c0 + cols]), (seg_pixels, win)


@pytest.mark.parametrize("shape", LATENTS)
@pytest.mark.parametrize("ver", VERSIONS)
def test_window_decode_is_the_slice_of_the_full_decode(codec, latents, priors, ver, shape):
    """Segments longer than a row (S = 32 and 100 on 13x15 and 5x7), windows that start and end
    mid-segment, S = 1, and a single segment per image (S = 65535)."""
    calls = _use(codec, priors, ver)
    h8, w8 = shape
    for S in SEG_PIXELS:
        wins = windows_of(h8, w8)
        assert segments(h8, w8, S, (0, 0, h8, w8)) == (_lib.NIC_OK, -(-h8 * w8 // S))
        _check_windows(latents[shape], S, calls, wins)


@pytest.mark.parametrize("ver", VERSIONS)
def test_window_decode_of_a_trained_latent(codec, priors, ver, golden, weights_trained):
    """The 64x96 latent of kodim21_full under the trained coef-0.01 encoder, seg_pixels 32."""
    c = Codec(0)
    try:
        c.set_weights({k: v for k, v in weights_trained.items() if k.startswith("encoder")})
        z = c.encode(_dev(golden("kodim21_full")["x"])).cpu().numpy()
    finally:
        c.close()
    assert z.shape == (1, 64, 96, 96)
    _check_windows(z, 32, _use(codec, priors, ver), windows_of(64, 96) + [(29, 5, 6, 70), (3, 90, 58, 6)])


@pytest.mark.parametrize("ver", VERSIONS)
def test_no_store_outside_the_output(codec, latents, priors, ver):
    z = latents[(13, 15)]
    encode, decode_status, window_status, _ = _use(codec, priors, ver)
    for S, win in ((7, (2, 3, 9, 8)), (100, (12, 14, 1, 1)), (1, (0, 0, 13, 15))):
        buf, sizes = encode(_dev(z), S)
        count = 3 * win[2] * win[3] * 96
        pad = 4096
        big = torch.full((pad + count + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[pad:pad + count].view(3, win[2], win[3], 96)
        got, status = window_status(buf, sizes, 13, 15, win, out=out)
        assert got.data_ptr() == out.data_ptr() and status.cpu().tolist() == [0, 0, 0]
        np.testing.assert_array_equal(out.cpu().numpy(), z[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
        assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + count:] == 0xA5).all())


@pytest.mark.parametrize("ver", VERSIONS)
def test_statuses(codec, priors, golden, ver):
    """Four 16x16 latents at seg_pixels 32: segment k is latent rows 2k and 2k + 1."""
    z = golden("imagenet4_trained")["latent"]
    encode, decode_status, window_status, _ = _use(codec, priors, ver)
    parse = {1: R.parse_file, 2: lambda d: R2.parse_file(d, priors[0]), 3: lambda d: R3.parse_file(d, priors[1])}[ver]
    buf, sizes = encode(_dev(z))
    host, sizes_h = buf.cpu().numpy().copy(), sizes.cpu().numpy()
    # a header of another geometry: 2
    assert window_status(buf, sizes, 8, 32, (1, 2, 3, 4))[1].cpu().tolist() == [2] * 4
    # a payload byte flipped in segment 3 (latent rows 6 and 7) of image 1
    info = parse(host[1, :sizes_h[1]].tobytes())
    k = 3
    host[1, info["payload"] + sum(info["seg_lengths"][:k]) + info["seg_lengths"][k] // 2] ^= 0x5A
    bad = _dev(host)
    assert decode_status(bad, sizes, 16, 16)[1].cpu().tolist() == [0, 1, 0, 0]      # the full decode sees it
    for win in ((0, 2, 6, 9), (8, 0, 8, 16)):                                         # windows beside segment 3: it is not decoded
        got, status = window_status(bad, sizes, 16, 16, win)
        assert status.cpu().tolist() == [0, 0, 0, 0], win
        np.testing.assert_array_equal(got.cpu().numpy(), z[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    for win in ((5, 2, 2, 9), (7, 15, 1, 1), (0, 0, 16, 16)):                         # windows that hold a pixel of it
        got, status = window_status(bad, sizes, 16, 16, win)
        assert status.cpu().tolist() == [0, 1, 0, 0], win
        keep = [0, 2, 3]
        np.testing.assert_array_equal(got.cpu().numpy()[keep], z[keep, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    decode_window = {1: codec.rans_decode_window, 2: codec.rans2_decode_window, 3: codec.rans3_decode_window}[ver]
    with pytest.raises(ValueError, match="image 1"):
        decode_window(bad, sizes, 16, 16, (5, 2, 2, 9))
    assert torch.equal(decode_window(bad, sizes, 16, 16, (0, 2, 6, 9)), _dev(z[:, 0:6, 2:11]))
    with pytest.raises(ValueError):                                                   # a window outside the latent
        window_status(buf, sizes, 16, 16, (10, 0, 7, 1))
    if ver == 1:
        return
    # another prior's file: 8, and nothing of it is written
    other = R2.uniform_prior() if ver == 2 else R3.uniform_context_prior()
    if ver == 2:
        codec.set_prior(Prior(other))
    else:
        codec.set_context_prior(ContextPrior(*other))
    out = torch.full((4, 3, 5, 96), 0xA5, dtype=torch.uint8, device="cuda")
    _, status = window_status(buf, sizes, 16, 16, (4, 4, 3, 5), out=out)
    assert status.cpu().tolist() == [8] * 4
    assert bool((out == 0xA5).all())
    with pytest.raises(ValueError, match="written under prior"):
        decode_window(buf, sizes, 16, 16, (4, 4, 3, 5))
    # and without a prior
    codec.set_prior(None)
    codec.set_context_prior(None)
    with pytest.raises(_lib.NicError) as e:
        window_status(buf, sizes, 16, 16, (4, 4, 3, 5))
    assert e.value.code == _lib.NIC_ENOPRIOR


# ---- end to end ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def coded(golden, weights_trained, weights_spread):
    """kodim21_full under the trained and the spread weights as version-1 and version-3 files, and its
    509 x 761 crop as a version-3 file that records its size: name -> (weights, file, (H, W))."""
    x = golden("kodim21_full")["x"]
    out = {}
    for wname, w in (("trained", weights_trained), ("spread", weights_spread)):
        c = Codec(0)
        try:
            c.set_weights({k: v for k, v in w.items() if k.startswith("encoder")})
            z = c.encode(_dev(x))
            zc = c.encode(_dev(x[:, :509, :761]))
            out[wname, 1] = (w, B.nic_files(c, z)[0], (512, 768), None)
            static = Prior.accumulator(c).add(z).build()
            cprior = ContextPrior.accumulator(c, static).add(z).build()
            c.set_context_prior(cprior)
            out[wname, 3] = (w, B.nic_files(c, z, size=(512, 768))[0], (512, 768), cprior)
            out[wname, "crop"] = (w, B.nic_files(c, zc, size=(509, 761))[0], (509, 761), cprior)
        finally:
            c.close()
    return out


def _decoder(w, cprior, precision):
    dec = Decoder(0, precision=precision)
    dec.set_weights(w)
    if cprior is not None:
        dec.codec.set_context_prior(cprior)
    return dec


def _whole(dec, data):
    (z,), (hw,) = B.read_nic(dec.codec, [data], sizes=True)
    return dec.codec.decode(z[None])[:, :hw[0], :hw[1]]


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("which", [("trained", 1), ("trained", 3), ("trained", "crop"), ("spread", 1), ("spread", 3),
                                   ("spread", "crop")], ids=lambda w: f"{w[0]}-{w[1]}")
def test_decode_region_is_the_crop_of_the_whole_decode(coded, which, precision):
    w, data, (H, W), cprior = coded[which]
    dec = _decoder(w, cprior, precision)
    try:
        whole = _whole(dec, data)
        assert tuple(whole.shape) == (1, H, W, 3)
        boxes = [(0, 0, 8, 8), (13, 21, 100, 77), (H - 40, W - 40, 40, 40), (200, 0, 16, W), (0, 0, H, W)]
        for y, x, h, w_ in boxes:
            got = dec.decode_region([data], (y, x, h, w_))
            assert tuple(got.shape) == (1, h, w_, 3) and got.is_contiguous()
            ref = whole[:, y:y + h, x:x + w_]
            diff = int((got != ref).sum())
            print(f"{which} {precision} box {(y, x, h, w_)}: {diff} differing bytes")
            assert diff == 0, (y, x, h, w_)
        for box in ((0, 0, H + 1, 8), (H - 7, 0, 8, 8), (0, W - 7, 8, 8), (-1, 0, 8, 8), (0, 0, 0, 8)):
            with pytest.raises(ValueError, match="file 0.*does not lie inside"):
                dec.decode_region([data], box)
    finally:
        dec.codec.close()


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_decode_region_where_window_and_frame_take_other_kernel_forms(weights_spread, precision, tmp_path, golden):
    """Two 40x70 parts of kodim21_full's spread-weight latent and the 10x12 latent pixels in their
    middle (a 16x18 window with the halo): the frame and the window run different forms of the k3
    layers.  Two files, one of them by path."""
    zf = golden("kodim21_full")["latent"]
    z = np.ascontiguousarray(np.concatenate([zf[:, :40, :70], zf[:, 24:, 26:]]))
    dec = _decoder(weights_spread, None, precision)
    try:
        files = B.nic_files(dec.codec, _dev(z))
        (tmp_path / "b.nic").write_bytes(files[1])
        box = (8 * 12, 8 * 20, 80, 96)
        assert Codec.region_plan(320, 560, box) == ((9, 17, 16, 18), (24, 24))
        whole = dec.codec.decode(_dev(z))
        got = dec.decode_region([files[0], str(tmp_path / "b.nic")], box)
        ref = whole[:, box[0]:box[0] + box[2], box[1]:box[1] + box[3]]
        diff = int((got != ref).sum())
        print(f"40x70 {precision}: {diff} differing bytes of {ref.numel()}")
        assert diff == 0
        # the files of one call decode as one batch
        other = B.nic_files(dec.codec, _dev(z[:1, :39]))
        with pytest.raises(ValueError, match="file 1.*39x70.*40x70"):
            dec.decode_region([files[0], other[0]], (0, 0, 8, 8))
        with pytest.raises(ValueError, match="b.nic"):
            dec.decode_region([str(tmp_path / "b.nic")], (0, 0, 321, 8))
    finally:
        dec.codec.close()


# ---- the directory drivers ------------------------------------------------------------------------

def _pixels(path):
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im)


def _read_dir(d):
    return {fn: (d / fn).read_bytes() for fn in sorted(os.listdir(d))}


@pytest.mark.parametrize("with_prior", [False, True], ids=["version1", "version3"])
def test_drivers_write_the_region(tmp_path, golden, weights_trained, with_prior):
    from PIL import Image

    from neural_network_image_compression_amd import weights as W
    ds = tmp_path / "imgs"
    ds.mkdir()
    g = golden("imagenet4")
    images = {"a0": np.ascontiguousarray(g["x"][0][32:96, 16:80]), "b_odd": golden("odd37x53")["x"][0],
              "c0": np.ascontiguousarray(g["x"][2][:61, :50])}
    for name, a in images.items():
        Image.fromarray(np.ascontiguousarray(a)).save(ds / f"{name}.png")
    ck = tmp_path / "ck"
    W.save(weights_trained, str(ck / "encoder"), "encoder")
    W.save(weights_trained, str(ck / "decoder"), "decoder")
    enc, dec = Encoder(0), Decoder(0)
    enc.load(str(ck / "encoder"))
    more = {}
    if with_prior:
        zs = [enc.codec.encode(_dev(a[None])) for a in images.values()]
        acc = Prior.accumulator(enc.codec)
        for z in zs:
            acc.add(z)
        cacc = ContextPrior.accumulator(enc.codec, acc.build())
        for z in zs:
            cacc.add(z)
        more = {"prior": cacc.build()}
    enc.compress(str(ds), str(ck / "encoder"), container="nic", **more)
    comp, out = tmp_path / "imgs_compressed", tmp_path / "imgs_uncompressed"
    assert all((comp / f"{n}.nic").read_bytes()[4] == (3 if with_prior else 1) for n in images)
    dec.uncompress(str(comp), str(ck / "decoder"), container="nic", **more)
    plain = _read_dir(out)
    whole = {n: _pixels(out / f"{n}.png") for n in images}
    # region=None is the call without the argument
    dec.uncompress(str(comp), str(ck / "decoder"), container="nic", region=None, **more)
    assert _read_dir(out) == plain
    box = (5, 9, 30, 40)  # inside the smallest image, 37 x 53
    for writer in B.PNG_WRITERS:
        for fn in os.listdir(out):
            os.remove(out / fn)
        dec.uncompress(str(comp), str(ck / "decoder"), container="nic", png_writer=writer, region=box, **more)
        assert sorted(os.listdir(out)) == sorted(n + ".png" for n in images)
        for n in images:
            got = _pixels(out / f"{n}.png")
            assert got.shape == (30, 40, 3)
            np.testing.assert_array_equal(got, whole[n][5:35, 9:49], f"{n} {writer}")
    # a box that one file's image does not hold: version-1 files stand for 8 h8 x 8 w8 = 40 x 56 pixels
    for fn in os.listdir(out):
        os.remove(out / fn)
    with pytest.raises(ValueError, match=r"b_odd\.nic.*does not lie inside"):
        dec.uncompress(str(comp), str(ck / "decoder"), container="nic", region=(0, 0, 41, 41), **more)
    if with_prior:  # the recorded 37 x 53
        with pytest.raises(ValueError, match=r"b_odd\.nic.*37 x 53"):
            dec.uncompress(str(comp), str(ck / "decoder"), container="nic", region=(0, 0, 38, 40), **more)
    assert os.listdir(out) == []
    # a damaged segment inside the region's window: the device's refusal is reported with the file's name
    d = bytearray((comp / "c0.nic").read_bytes())
    info = R3.parse_file(bytes(d)) if with_prior else R.parse_file(bytes(d))
    d[info["payload"] + info["seg_lengths"][0] // 2] ^= 0x5A
    whole_c0 = (comp / "c0.nic").read_bytes()
    (comp / "c0.nic").write_bytes(bytes(d))
    with pytest.raises(ValueError, match=r"imgs_compressed: c0\.nic: .*image 0 is corrupt"):
        dec.uncompress(str(comp), str(ck / "decoder"), container="nic", region=(0, 0, 8, 8), **more)
    (comp / "c0.nic").write_bytes(whole_c0)
    # a packed PNG has no index
    with pytest.raises(ValueError, match="region"):
        dec.uncompress(str(comp), str(ck / "decoder"), region=box)
    with pytest.raises(ValueError, match="region"):
        B.use_model(enc, str(ds), str(ck / "encoder"), str(tmp_path / "x"), in_cshape=3, container="nic", region=box)
