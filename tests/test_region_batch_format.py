"""CPU checks of batched region decode's host side: nic_region_plan_fixed against the properties that
make its windows batchable and its cut exact, the plan's exactness on the NumPy oracle, and the
argument checks of nic_rans*_decode_windows and nic_cut_boxes (no GPU calls here)."""
import ctypes

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from oracle import nic_oracle as O
from tests.test_region_format import HALO, plan

# the latents and boxes shared with tests/test_gpu_region_batch.py
BOX = (40, 24)  # (h, w): R = 40 // 8 + 1 + 1 + 6 = 12 latent rows, C = (24 + 6) // 8 + 1 + 6 = 10 latent columns
LATENTS = ((13, 15), (20, 9), (40, 70), (32, 32))


def boxes_of(h8, w8, bh=BOX[0], bw=BOX[1]):
    """The four corners, the middle of the left edge, and an unaligned interior position, of an 8 h8 x 8 w8 image."""
    H, W = 8 * h8, 8 * w8
    return [(0, 0, bh, bw), (0, W - bw, bh, bw), (H - bh, 0, bh, bw), (H - bh, W - bw, bh, bw),
            ((H - bh) // 2 + 1, 0, bh, bw), ((H - bh) // 2 - 3, (W - bw) // 2 + 5, bh, bw)]


def plan_fixed(H, W, y, x, bh, bw):
    win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
    rc = _lib.lib().nic_region_plan_fixed(H, W, y, x, bh, bw, win, off)
    return rc, tuple(win), tuple(off)


def fixed_count(len_, n8):
    """nic.h's rule for one axis: the most latent pixels len_ image pixels touch, the halo on both sides, clamped."""
    return min(n8, (len_ + 6) // 8 + 1 + 2 * HALO)


def test_fixed_plan_properties():
    """H, W in {8, 37, 64, 100, 203}, bh, bw in {1, 8, 9, 40}, every y, every seventh x and the last."""
    sizes, lens = (8, 37, 64, 100, 203), (1, 8, 9, 40)
    shape_of = {}  # (bh, bw, min(h8, R), min(w8, C)) -> the one window shape seen under it
    checked = shifted = 0
    for H in sizes:
        for W in sizes:
            h8, w8 = -(-H // 8), -(-W // 8)
            for bh in lens:
                for bw in lens:
                    if bh > H or bw > W:
                        assert plan_fixed(H, W, 0, 0, bh, bw)[0] == plan(H, W, 0, 0, bh, bw)[0] == _lib.NIC_ESHAPE
                        continue
                    key = (bh, bw, fixed_count(bh, h8), fixed_count(bw, w8))
                    for y in range(H - bh + 1):
                        for x in sorted(set(range(0, W - bw + 1, 7)) | {W - bw}):
                            rc, (r0, c0, rows, cols), off = plan_fixed(H, W, y, x, bh, bw)
                            rc1, (p0, q0, prows, pcols), _ = plan(H, W, y, x, bh, bw)
                            assert rc == rc1 == _lib.NIC_OK
                            box = (H, W, y, x, bh, bw)
                            assert (rows, cols) == key[2:], box
                            assert shape_of.setdefault(key, (rows, cols)) == (rows, cols), box
                            assert 0 <= r0 and r0 + rows <= h8 and 0 <= c0 and c0 + cols <= w8, box
                            # it holds nic_region_plan's window
                            assert r0 <= p0 and p0 + prows <= r0 + rows and c0 <= q0 and q0 + pcols <= c0 + cols, box
                            # an edge is the frame's, or at least the halo beyond the latent pixels the box touches
                            assert r0 == 0 or r0 <= y // 8 - HALO, box
                            assert r0 + rows == h8 or r0 + rows >= (y + bh - 1) // 8 + 1 + HALO, box
                            assert c0 == 0 or c0 <= x // 8 - HALO, box
                            assert c0 + cols == w8 or c0 + cols >= (x + bw - 1) // 8 + 1 + HALO, box
                            assert off == (y - 8 * r0, x - 8 * c0), box
                            assert off[0] >= 0 and off[0] + bh <= 8 * rows and off[1] >= 0 and off[1] + bw <= 8 * cols, box
                            shifted += (r0, c0) != (p0, q0)
                            checked += 1
    assert checked > 100000 and shifted > 1000  # and the clamp did move windows
    assert _lib.lib().nic_version() >= 800


def test_fixed_plan_refuses_what_region_plan_refuses():
    H, W = 37, 53
    for box in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -3, 4), (34, 0, 4, 4), (0, 50, 4, 4),
                (37, 0, 1, 1), (0, 53, 1, 1), (0, 0, 38, 53), (0, 0, 37, 54), (1, 0, 2 ** 31 - 1, 1), (0, 1, 1, 2 ** 31 - 1)):
        assert plan(H, W, *box)[0] == _lib.NIC_ESHAPE
        assert plan_fixed(H, W, *box)[0] == _lib.NIC_ESHAPE, box
        assert "nic_region_plan_fixed" in _lib.last_error()
    for H_, W_ in ((0, 8), (8, -8)):
        assert plan_fixed(H_, W_, 0, 0, 1, 1)[0] == plan(H_, W_, 0, 0, 1, 1)[0] == _lib.NIC_ESHAPE
    L = _lib.lib()
    win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
    assert L.nic_region_plan_fixed(H, W, 0, 0, 4, 4, None, off) == _lib.NIC_EINVAL
    assert L.nic_region_plan_fixed(H, W, 0, 0, 4, 4, win, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()
    # hand-checked: a 1 x 1 box needs 1 + 6 = 7 latent pixels per axis, the 37 x 53 image has 5 x 7
    assert plan_fixed(H, W, 36, 52, 1, 1) == (_lib.NIC_OK, (0, 0, 5, 7), (36, 52))
    # and in a 203 x 203 image (26 x 26) the window of the last pixel ends on the frame: 26 - 7 = 19
    assert plan_fixed(203, 203, 202, 202, 1, 1) == (_lib.NIC_OK, (19, 19, 7, 7), (50, 50))
    assert plan(203, 203, 202, 202, 1, 1)[1] == (22, 22, 4, 4)


@pytest.mark.parametrize("h8,w8", [(13, 15), (20, 9)])
def test_the_fixed_plan_is_exact_on_the_oracle(weights_spread, h8, w8):
    """The oracle's decode of the fixed window, cut at off2, is the crop of its decode of the whole
    latent, bit for bit: the corners and the edge, where the clamp shifts the window inward and it
    reaches further from the box than the halo, and the interior."""
    H, W = 8 * h8, 8 * w8
    z = np.random.default_rng(11).integers(0, 256, (1, h8, w8, 96), dtype=np.uint8)
    whole = O.decode(weights_spread, z)
    assert whole.shape == (1, H, W, 3)
    shifted = 0
    for y, x, bh, bw in boxes_of(h8, w8) + boxes_of(h8, w8, 9, 17)[3:]:
        rc, (r0, c0, rows, cols), (oy, ox) = plan_fixed(H, W, y, x, bh, bw)
        assert rc == _lib.NIC_OK and (rows, cols) == (fixed_count(bh, h8), fixed_count(bw, w8))
        shifted += (r0, c0) != plan(H, W, y, x, bh, bw)[1][:2]
        part = O.decode(weights_spread, np.ascontiguousarray(z[:, r0:r0 + rows, c0:c0 + cols]))
        np.testing.assert_array_equal(part[:, oy:oy + bh, ox:ox + bw], whole[:, y:y + bh, x:x + bw], str((y, x, bh, bw)))
    assert shifted >= 3
    assert (fixed_count(BOX[0], h8), fixed_count(BOX[1], w8)) == ((12, 10) if (h8, w8) == (13, 15) else (12, 9))


@pytest.mark.parametrize("name", ["nic_rans_decode_windows", "nic_rans2_decode_windows", "nic_rans3_decode_windows"])
def test_decode_windows_validates_without_a_gpu(name):
    # shape, empty batch, then NULL, all before any HIP call (the table lives on the device and is checked there)
    f = getattr(_lib.lib(), name)
    big = 1 << 20
    assert f(None, None, big, None, 1, None, 16, 4, 4, None, None, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error() and name + ":" in _lib.last_error()
    for n, max_pixels, rows, cols in ((-1, 16, 4, 4), (65536, 16, 4, 4), (1, 0, 1, 1), (1, (1 << 23) + 1, 1, 1), (1, 16, 0, 4),
                                      (1, 16, 4, 0), (1, 16, -1, 4), (1, 16, 4, 5), (1, 16, 17, 1), (1, 1 << 23, 1 << 16, 1 << 16)):
        assert f(None, None, big, None, n, None, max_pixels, rows, cols, None, None, None) == _lib.NIC_ESHAPE, (n, max_pixels, rows, cols)
    assert f(None, None, 0, None, 0, None, 16, 0, 4, None, None, None) == _lib.NIC_ESHAPE  # before the empty batch
    assert f(None, None, 0, None, 0, None, 16, 4, 4, None, None, None) == _lib.NIC_OK  # empty batch


def test_cut_boxes_validates_without_a_gpu():
    f = _lib.lib().nic_cut_boxes
    assert f(None, None, 1, 8, 8, None, 4, 4, None, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error() and "nic_cut_boxes:" in _lib.last_error()
    for n, Hs, Ws, bh, bw in ((-1, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 0, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0), (1, 8, 8, 9, 4),
                              (1, 8, 8, 4, 9), (1, 1 << 15, 1 << 15, 4, 4)):
        assert f(None, None, n, Hs, Ws, None, bh, bw, None, None) == _lib.NIC_ESHAPE, (n, Hs, Ws, bh, bw)
    assert f(None, None, 0, 8, 8, None, 9, 4, None, None) == _lib.NIC_ESHAPE  # before the empty batch
    assert f(None, None, 0, 8, 8, None, 8, 8, None, None) == _lib.NIC_OK  # empty batch
