"""The device rANS coder of the .nic container (csrc/nic_rans.hip) against the pure-Python
reference (tests/rans_ref.py): round trips over every code path (partial segments and waves,
dense and single-symbol tables, the normalisation corner cases), file conformance in both
directions, determinism and batch invariance, coding efficiency, a corrupt payload, and the
directory drivers with container="nic"."""
import ctypes
import os

import numpy as np
import pytest

from oracle import nic_oracle as O
from tests import rans_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import _lib  # noqa: E402
from neural_network_image_compression_amd import bitstream as B  # noqa: E402
from neural_network_image_compression_amd.codec import Codec, Decoder, Encoder  # noqa: E402

TRAINED_256 = ("kodim21_256_trained", "kodim21_256_trained_c0.02", "kodim21_256_trained_c0.03")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def codec():
    c = Codec(0)  # the coder needs no weights
    yield c
    c.close()


@pytest.fixture(scope="module")
def latents(golden):
    """The cases of the issue: (a) 1x1, (b) odd 5x7 dense, (c) three trained 32x32 as one batch,
    (d) 2 x 72x72 with four crafted channels and the rest random skewed."""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (1, 1, 1, 96), dtype=np.uint8)
    b = golden("odd37x53")["latent"]
    c = np.concatenate([golden(k)["latent"] for k in TRAINED_256])
    npix = 72 * 72
    d = np.minimum(rng.geometric(0.15, (2, npix, 96)) - 1, 255).astype(np.uint8)
    for i in range(2):
        d[i, :, 0] = (np.arange(npix) + 3 * i) % 256                # cycles all 256 symbols
        d[i, :, 1] = 255                                              # constant: freq 4096
        d[i, :, 2] = 7                                                # one symbol once among 5,183 of another
        d[i, 1234 + i, 2] = 200
        ch3 = np.concatenate([np.arange(200), 200 + np.arange(npix - 200) % 56])  # 200 singletons + 56 sharing the rest
        d[i, :, 3] = rng.permutation(ch3)
    d = d.reshape(2, 72, 72, 96)
    assert c.shape == (3, 32, 32, 96) and b.shape == (1, 5, 7, 96)
    return {"a": a, "b": b, "c": c, "d": d}


@pytest.fixture(scope="module")
def files_c(codec, latents):
    """Batch (c)'s device files at the default seg_pixels, shared by the tests below."""
    return B.nic_files(codec, _dev(latents["c"]))


def _payload_check(z, data):
    info = R.parse_file(data)
    nseg = len(info["seg_lengths"])
    payload, ideal = sum(info["seg_lengths"]), R.ideal_payload_bytes(z, info["tables"])
    print(f"file {len(data)} tables {info['table_bytes']} payload {payload} ideal {ideal:.1f} nseg {nseg}")
    assert payload <= ideal + 5 * nseg  # 4 state bytes + 1 byte of granularity per segment


@pytest.mark.parametrize("case,seg_pixels", [("a", 32), ("b", 32), ("c", 32), ("d", 32), ("b", 1), ("b", 4096), ("c", 1),
                                             ("c", 4096)])
def test_round_trip(codec, latents, case, seg_pixels):
    z = latents[case]
    n, h8, w8, _ = z.shape
    zd = _dev(z)
    buf, sizes = codec.rans_encode(zd, seg_pixels)
    back, status = codec.rans_decode_status(buf, sizes, h8, w8)
    assert status.cpu().tolist() == [0] * n
    np.testing.assert_array_equal(back.cpu().numpy(), z)
    np.testing.assert_array_equal(codec.rans_decode(buf, sizes, h8, w8).cpu().numpy(), z)
    # the files are well formed and of the advertised geometry
    sizes_h, host = sizes.cpu().numpy(), buf.cpu().numpy()
    bound = ctypes.c_int64()
    assert _lib.lib().nic_rans_bound(h8, w8, seg_pixels, ctypes.byref(bound)) == 0 and buf.shape[1] == bound.value
    for i in range(n):
        data = host[i, :sizes_h[i]].tobytes()
        assert B.nic_inspect(data) == (h8, w8, seg_pixels)
        _payload_check(z[i], data)


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_conformance_with_the_reference(codec, latents, files_c, case):
    z = latents[case]
    files = files_c if case == "c" else B.nic_files(codec, _dev(z))
    imgs = range(len(z)) if case != "d" else [0]  # (d): one image through the Python coder keeps the test short
    for i in imgs:
        # GPU file -> reference reader
        np.testing.assert_array_equal(R.read_file(files[i]), z[i])
        # the reference writer fed the GPU file's tables reproduces the GPU file
        tables = R.parse_file(files[i])["tables"]
        assert R.write_file(z[i], 32, tables) == files[i]
    for i in range(len(z)):
        # the device normalisation is the documented one, which rans_ref restates
        assert R.parse_file(files[i])["tables"] == R.tables_of_latent(z[i])
    # reference-written files (its own tables, other segment sizes too) -> GPU reader
    sp = {"a": 32, "b": 3, "c": 32, "d": 100}[case]
    ref = [R.write_file(z[i], sp) for i in imgs]
    back = B.read_nic(codec, ref)
    for k, i in enumerate(imgs):
        np.testing.assert_array_equal(back[k].cpu().numpy(), z[i])


def test_crafted_channels_normalise_as_specified(codec, latents):
    data = B.nic_files(codec, _dev(latents["d"]))[1]
    t = R.parse_file(data)["tables"]
    assert sum(1 for v in t[0] if v) == 256 and min(t[0]) >= 1            # all 256 symbols
    assert t[1][255] == 4096 and sum(1 for v in t[1] if v) == 1           # constant channel
    assert t[2][200] == 1 and t[2][7] == 4095                             # floor-to-zero bump
    assert all(t[3][s] == 1 for s in range(200)) and sum(t[3]) == 4096    # overshoot spread over the large entries
    assert min(t[3][200:]) >= 1 and max(t[3][200:]) - min(t[3][200:]) <= 1


def test_deterministic_and_batch_invariant(codec, latents, files_c):
    assert B.nic_files(codec, _dev(latents["c"])) == files_c
    for i in range(3):
        assert B.nic_files(codec, _dev(latents["c"][i:i + 1])) == [files_c[i]]


def test_trained_files_are_smaller_than_the_png(latents, files_c):
    for i, case in enumerate(TRAINED_256):
        png = len(B.png_bytes(O.pack_latent(latents["c"][i:i + 1])[0]))
        print(f"{case}: nic {len(files_c[i])} png {png}")
        assert len(files_c[i]) < png


def test_corrupt_payload_is_reported_per_image(codec, latents):
    z = latents["c"]
    buf, sizes = codec.rans_encode(_dev(z))
    host, sizes_h = buf.cpu().numpy().copy(), sizes.cpu().numpy()
    info = R.parse_file(host[1, :sizes_h[1]].tobytes())
    k = 17  # one payload byte in the middle of segment 17 of image 1; every length stays intact
    at = info["payload"] + sum(info["seg_lengths"][:k]) + info["seg_lengths"][k] // 2
    host[1, at] ^= 0x5A
    assert B.nic_inspect(host[1, :sizes_h[1]].tobytes()) == (32, 32, 32)  # the container itself is still well formed
    bad = _dev(host)
    back, status = codec.rans_decode_status(bad, sizes, 32, 32)
    st = status.cpu().tolist()
    assert st[0] == 0 and st[1] != 0 and st[2] == 0
    np.testing.assert_array_equal(back[0].cpu().numpy(), z[0])
    np.testing.assert_array_equal(back[2].cpu().numpy(), z[2])
    with pytest.raises(ValueError, match="image 1"):
        codec.rans_decode(bad, sizes, 32, 32)


def test_foreign_header_is_refused_on_the_device(codec, latents):
    buf, sizes = codec.rans_encode(_dev(latents["b"]))
    with pytest.raises(ValueError, match="image 0"):
        codec.rans_decode(buf, sizes, 7, 5)  # the files hold 5 x 7 latents
    with pytest.raises(ValueError, match="nic_rans_inspect"):
        B.read_nic(codec, [b"NICR" + bytes(40)])


def test_drivers_with_the_nic_container(tmp_path, golden, weights_trained):
    from PIL import Image

    from neural_network_image_compression_amd import weights as W
    ds = tmp_path / "imgs"
    ds.mkdir()
    g = golden("imagenet4")
    crops = [np.ascontiguousarray(g["x"][i][32:96, 16:80]) for i in range(4)]
    odd = golden("odd37x53")["x"][0]
    for name, a in (("a0", crops[0]), ("a1", crops[1]), ("b_odd", odd), ("c0", crops[2]), ("c1", crops[3])):
        Image.fromarray(a).save(ds / f"{name}.png")
    W.save(weights_trained, str(tmp_path / "ck" / "encoder"), "encoder")
    W.save(weights_trained, str(tmp_path / "ck" / "decoder"), "decoder")
    enc, dec = Encoder(0), Decoder(0)
    enc.compress(str(ds), str(tmp_path / "ck" / "encoder"), container="nic")
    names = ["a0", "a1", "b_odd", "c0", "c1"]
    assert sorted(os.listdir(tmp_path / "imgs_compressed")) == [n + ".nic" for n in names]
    # every file is nic_files of codec.encode of its image
    for name, a in zip(names, (crops[0], crops[1], odd, crops[2], crops[3])):
        want, = B.nic_files(enc.codec, enc.codec.encode(_dev(a[None])))
        assert (tmp_path / "imgs_compressed" / f"{name}.nic").read_bytes() == want
    dec.uncompress(str(tmp_path / "imgs_compressed"), str(tmp_path / "ck" / "decoder"), container="nic")
    # the default PNG route, from the same images
    ds2 = tmp_path / "pngroute"
    ds2.mkdir()
    for n in names:
        (ds2 / f"{n}.png").write_bytes((ds / f"{n}.png").read_bytes())
    enc.compress(str(ds2), str(tmp_path / "ck" / "encoder"))
    dec.uncompress(str(tmp_path / "pngroute_compressed"), str(tmp_path / "ck" / "decoder"))
    assert sorted(os.listdir(tmp_path / "imgs_uncompressed")) == [n + ".png" for n in names]
    for n in names:
        assert (tmp_path / "imgs_uncompressed" / f"{n}.png").read_bytes() == \
            (tmp_path / "pngroute_uncompressed" / f"{n}.png").read_bytes(), n
    # the serial driver writes the same files
    dec.uncompress(str(tmp_path / "imgs_compressed"), str(tmp_path / "ck" / "decoder"), container="nic", workers=0,
                   batch_size=2)
    for n in names:
        assert (tmp_path / "imgs_uncompressed" / f"{n}.png").read_bytes() == \
            (tmp_path / "pngroute_uncompressed" / f"{n}.png").read_bytes(), n
