"""CPU-side checks of the device PNG writer (DESIGN.md "The device PNG writer"): the test reader
tests/png_parse.py against a Pillow file, the bound formula, the block size, the argument checks
that come before any GPU call, and the png_writer keyword."""
import ctypes

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from neural_network_image_compression_amd import bitstream as B
from neural_network_image_compression_amd.codec import Decoder
from tests import png_parse as P

FRAMING = 8 + 25 + 8 + 2 + 4 + 4 + 12  # signature, IHDR, IDAT length + type, zlib header, Adler-32, CRC, IEND


def bound_formula(h, w, channels, block_bytes):
    """the framing, every block stored (5 bytes of stored-block header each)."""
    total = h * (w * channels + 1)
    return FRAMING + total + 5 * ((total + block_bytes - 1) // block_bytes)


def test_reader_round_trips_a_pillow_file(golden):
    from PIL import Image
    import io

    recon = golden("odd37x53")["recon"][0]
    assert recon.shape == (40, 56, 3)
    data = B.png_bytes(recon)
    png = P.parse(data)
    assert (png.width, png.height, png.bit_depth, png.colour_type, png.interlace) == (56, 40, 8, 2, 0)
    assert [c[0] for c in png.chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert len(png.filtered) == 40 * (56 * 3 + 1) and set(png.filter_bytes()) <= {0, 1, 2, 3, 4}
    blocks = P.deflate_blocks(png.idat)
    assert blocks and blocks[-1]["final"] and all(not b["final"] for b in blocks[:-1])
    np.testing.assert_array_equal(np.array(Image.open(io.BytesIO(data))), recon)
    # a flipped bit in the IDAT data is caught by the chunk CRC
    bad = bytearray(data)
    bad[60] ^= 1
    with pytest.raises(AssertionError):
        P.parse(bytes(bad))


def test_block_bytes():
    assert _lib.lib().nic_png_device_block_bytes() >= 8192


@pytest.mark.parametrize("h,w,c", [(1, 1, 1), (1, 1, 3), (40, 56, 3), (256, 256, 3), (2160, 3840, 3)])
def test_bound_is_the_formula(h, w, c):
    L = _lib.lib()
    b = ctypes.c_int64()
    assert L.nic_png_device_bound(h, w, c, ctypes.byref(b)) == _lib.NIC_OK
    assert b.value == bound_formula(h, w, c, L.nic_png_device_block_bytes())


def test_arguments_are_checked_before_any_gpu_call():
    L = _lib.lib()
    b = ctypes.c_int64()
    assert L.nic_version() >= 400
    assert L.nic_png_device_bound(8, 8, 3, None) == _lib.NIC_EINVAL
    assert L.nic_png_device_bound(8, 8, 2, ctypes.byref(b)) == _lib.NIC_EINVAL
    assert L.nic_png_device_bound(0, 8, 3, ctypes.byref(b)) == _lib.NIC_ESHAPE
    assert L.nic_png_device_bound(8, 16385, 1, ctypes.byref(b)) == _lib.NIC_ESHAPE
    assert L.nic_png_device_bound(8, 16384, 1, ctypes.byref(b)) == _lib.NIC_OK
    assert L.nic_png_device_bound(8, 5462, 3, ctypes.byref(b)) == _lib.NIC_ESHAPE  # 16386 bytes per row
    assert L.nic_png_device_bound(8, 8, 3, ctypes.byref(b)) == _lib.NIC_OK
    bound = b.value
    p = ctypes.c_void_p(256)  # never dereferenced: the checks fail first
    enc = L.nic_png_device_encode
    assert enc(None, p, 1, 8, 8, 3, -1, p, bound, p, None) == _lib.NIC_EINVAL  # NULL ctx
    assert "NULL" in _lib.last_error()
    assert enc(None, None, 1, 8, 8, 3, -1, None, bound, None, None) == _lib.NIC_EINVAL
    assert enc(None, p, 1, 8, 8, 2, -1, p, bound, p, None) == _lib.NIC_EINVAL
    assert "channels" in _lib.last_error()
    assert enc(None, p, 1, 8, 8, 3, 5, p, bound, p, None) == _lib.NIC_EINVAL
    assert "filter" in _lib.last_error()
    assert enc(None, p, 1, 8, 8, 3, -2, p, bound, p, None) == _lib.NIC_EINVAL
    assert enc(None, p, 1, 8, 16385, 1, -1, p, 1 << 30, p, None) == _lib.NIC_ESHAPE
    assert enc(None, p, 1, 0, 8, 3, -1, p, bound, p, None) == _lib.NIC_ESHAPE
    assert enc(None, p, 1, 8, 8, 3, -1, p, bound - 1, p, None) == _lib.NIC_ESHAPE
    assert "stride" in _lib.last_error()
    assert enc(None, None, 0, 8, 8, 3, -1, None, 0, None, None) == _lib.NIC_OK  # empty batch
    assert L.nic_png_device_reserve(None, 1, 8, 8, 3) == _lib.NIC_EINVAL
    assert L.nic_png_device_reserve(None, 1, 8, 8, 2) == _lib.NIC_EINVAL
    assert L.nic_png_device_reserve(None, 1, 8, 16385, 1) == _lib.NIC_ESHAPE
    assert L.nic_png_device_reserve(None, 0, 8, 8, 3) == _lib.NIC_OK


def test_png_writer_keyword_is_checked_before_any_work(tmp_path):
    # no model is touched: the checks come first
    with pytest.raises(ValueError, match="png_writer"):
        B.use_model(None, str(tmp_path), "ck", str(tmp_path / "o"), in_cshape=96, png_writer="zlib")
    with pytest.raises(ValueError, match="png_writer"):
        B.use_model(None, str(tmp_path), "ck", str(tmp_path / "o"), in_cshape=96, container="nic", png_writer="zlib")
    with pytest.raises(ValueError, match="png_writer"):
        B.use_model_nic_in(None, str(tmp_path), "ck", str(tmp_path / "o"), png_writer="zlib")
    with pytest.raises(ValueError, match="png_writer"):
        Decoder.uncompress(object(), str(tmp_path / "x_compressed"), "ck", png_writer="Device")
    # the compress side's PNG is the reference bitstream
    for container in B.CONTAINERS:
        with pytest.raises(ValueError, match="decoder side"):
            B.use_model(None, str(tmp_path), "ck", str(tmp_path / "o"), in_cshape=3, container=container,
                        png_writer="device")
    assert not (tmp_path / "o").exists()
    assert B.PNG_WRITERS == ("pillow", "device")
