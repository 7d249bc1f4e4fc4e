"""CPU checks of the device PNG reader's host half: nic_png_inspect on Pillow's, the native writer's
and hand-built files (the framed edge streams of tests/png_read_cases.py among them, which Pillow
must read as the images they were built from), its unsupported and corrupt verdicts, the drivers'
option checks (which raise before any GPU call), and png_make's filters against Pillow."""
import ctypes
import io

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from neural_network_image_compression_amd import bitstream as B
from neural_network_image_compression_amd.codec import Decoder, Encoder
from PIL import Image

from tests import png_make as M
from tests import png_parse, png_read_cases as C


def inspect(data: bytes):
    a = np.frombuffer(data, np.uint8)
    h, w, ch, n = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    out = np.zeros(len(data) + 1, np.uint8)
    rc = _lib.lib().nic_png_inspect(a.ctypes.data_as(ctypes.c_void_p), len(data), ctypes.byref(h), ctypes.byref(w),
                                    ctypes.byref(ch), out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(n))
    return rc, (h.value, w.value, ch.value), out[:max(n.value, 0)].tobytes()


@pytest.mark.parametrize("name", sorted(C.format_files()))
def test_inspect_returns_shape_and_stream(name):
    data = C.format_files()[name]
    p = png_parse.parse(data)
    rc, shape, stream = inspect(data)
    assert rc == _lib.NIC_OK, _lib.last_error()
    assert shape == (p.height, p.width, p.channels)
    assert stream == p.idat
    assert B.png_stream(data) == (p.height, p.width, p.channels, p.idat)


def pillow_pixels(data: bytes) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im)


@pytest.mark.parametrize("name", sorted(n for n, v in C.edge_streams().items() if v[2] == 0))
def test_framed_edge_streams_are_files_pillow_and_inspect_take(name):
    """The GPU test's reference for an edge stream is Pillow's reading of the framed file: here it is
    the image the stream was built from, and nic_png_inspect hands the stream back unchanged."""
    stream, (h, w, ch), _ = C.edge_streams()[name]
    data = M.frame(h, w, ch, stream)
    rc, shape, got = inspect(data)
    assert rc == _lib.NIC_OK, _lib.last_error()
    assert shape == (h, w, ch) and got == stream
    assert np.array_equal(pillow_pixels(data), C.edge_image(name))


@pytest.mark.parametrize("f", range(5))
def test_png_make_filters_are_png_s(f):
    """filter_rows (Paeth vectorised) against Pillow's unfilter, RGB and grey, more than one row."""
    a = C.rgb_image(37, 53)
    g = np.ascontiguousarray(a[:, :, 1])
    assert np.array_equal(pillow_pixels(M.make_png(a, f)), a) and np.array_equal(pillow_pixels(M.make_png(g, f)), g)
    mixed = [(f + r) % 5 for r in range(37)]
    assert np.array_equal(pillow_pixels(M.make_png(a, mixed)), a)
    one = np.ascontiguousarray(a[:, :1])  # one pixel per row: no left neighbour anywhere
    assert np.array_equal(pillow_pixels(M.make_png(one, f)), one)


def test_idat_sizes_and_ancillary_chunks_really_occur():
    f = C.format_files()
    sizes = lambda name: [n for t, n in png_parse.parse(f[name]).chunks if t == b"IDAT"]  # noqa: E731
    assert set(sizes("make_idat1")) == {1} and len(sizes("make_idat1")) > 10
    assert set(sizes("make_idat7")[:-1]) == {7} and len(sizes("make_idat7")) > 10
    assert sizes("make_idat8192")[0] == 8192 and len(sizes("make_idat8192")) == 2
    assert len(sizes("native_tf")) >= 1 and len(sizes("pillow_rgb")) == 1
    assert [t for t, _ in png_parse.parse(f["make_chunks"]).chunks] == [b"IHDR", b"gAMA", b"pHYs", b"IDAT", b"tEXt", b"IEND"]


def test_sizes_only_and_short_buffer():
    data = C.format_files()["pillow_rgb"]
    a = np.frombuffer(data, np.uint8)
    n = ctypes.c_int64()
    L = _lib.lib()
    assert L.nic_png_inspect(a.ctypes.data_as(ctypes.c_void_p), len(data), None, None, None, None, 0, ctypes.byref(n)) == _lib.NIC_OK
    assert n.value == len(png_parse.parse(data).idat)
    out = np.zeros(4, np.uint8)
    assert L.nic_png_inspect(a.ctypes.data_as(ctypes.c_void_p), len(data), None, None, None, out.ctypes.data_as(ctypes.c_void_p),
                             4, None) == _lib.NIC_ESHAPE
    assert L.nic_png_inspect(None, 10, None, None, None, None, 0, None) == _lib.NIC_EINVAL


@pytest.mark.parametrize("name", sorted(C.unsupported_files()))
def test_unsupported_kinds_are_not_errors(name):
    data = C.unsupported_files()[name]
    png_parse.parse(data) if name != "interlaced" else None  # well-formed (png_parse does not de-interlace sizes)
    rc, _, _ = inspect(data)
    assert rc == _lib.NIC_EUNSUPPORTED, (rc, _lib.last_error())
    assert _lib.last_error().startswith("nic_png_inspect: ")
    with pytest.raises(B.PngUnsupported):
        B.png_stream(data)


@pytest.mark.parametrize("name", sorted(C.corrupt_files()))
def test_corrupt_files(name):
    data = C.corrupt_files()[name]
    rc, _, _ = inspect(data)
    assert rc == _lib.NIC_ECORRUPT, (rc, _lib.last_error())
    with pytest.raises(ValueError) as e:
        B.png_stream(data)
    assert not isinstance(e.value, B.PngUnsupported)
    with pytest.raises(ValueError, match="there.png"):
        B._png_item(data, "there.png")


def test_not_a_png():
    assert inspect(b"")[0] == _lib.NIC_ECORRUPT
    assert inspect(b"\xff\xd8\xff\xe0 not a png at all")[0] == _lib.NIC_ECORRUPT


def test_device_entry_points_validate_without_a_gpu():
    L = _lib.lib()
    assert L.nic_png_device_read(None, None, 16, None, 0, 8, 8, 3, None, None, None) == _lib.NIC_OK  # empty batch
    assert L.nic_png_device_read(None, None, 16, None, 1, 8, 8, 2, None, None, None) == _lib.NIC_EINVAL
    assert L.nic_png_device_read(None, None, 16, None, 1, 8, 16385, 1, None, None, None) == _lib.NIC_ESHAPE
    assert L.nic_png_device_read(None, None, 0, None, 1, 8, 8, 3, None, None, None) == _lib.NIC_ESHAPE
    assert L.nic_png_device_read(None, None, 16, None, 1, 8, 8, 3, None, None, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()
    assert L.nic_png_device_read_reserve(None, 1, 0, 8, 3) == _lib.NIC_ESHAPE
    assert L.nic_png_device_read_reserve(None, 1, 8, 8, 3) == _lib.NIC_EINVAL


class _NoGpu:
    """Stands where a ProClass would: any use of the model past the option checks is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the option check came after model.{name}")


def test_driver_option_checks_raise_before_any_gpu_call(tmp_path):
    with pytest.raises(ValueError, match="png_reader"):
        B.use_model(_NoGpu(), str(tmp_path), "ckpt", str(tmp_path / "out"), in_cshape=3, png_reader="gpu")
    with pytest.raises(ValueError, match="png_reader"):
        B.use_model(_NoGpu(), str(tmp_path), "ckpt", str(tmp_path / "out"), in_cshape=96, container="nic", png_reader="device")
    with pytest.raises(ValueError, match="png_reader"):
        Encoder.compress(_NoGpu(), str(tmp_path), "ckpt", png_reader="host")
    with pytest.raises(ValueError, match="png_reader"):
        Decoder.uncompress(_NoGpu(), str(tmp_path), "ckpt", container="nic", png_reader="device")
    assert not (tmp_path / "out").exists()
