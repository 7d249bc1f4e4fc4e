"""CPU checks of region decode's host side: nic_region_plan against a plain restatement of nic.h's
rule, the plan's exactness on the NumPy oracle (the planned window, decoded and cut, is the crop of
the whole decode), nic_rans_window_segments against a count over the window's pixels, and the
argument checks of the three nic_rans*_decode_window entry points (no GPU calls here)."""
import ctypes

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from oracle import nic_oracle as O

HALO = 3  # nic.h NIC_DECODE_HALO

# (h8, w8) latents, seg_pixels and windows shared with tests/test_gpu_region.py
LATENTS = ((13, 15), (5, 7), (40, 70), (1, 1))
SEG_PIXELS = (1, 7, 32, 100, 65535)


def windows_of(h8, w8):
    """Whole, single pixels at the corners and the centre, a full row, a full column, an interior box."""
    wins = {(0, 0, h8, w8), (0, 0, 1, 1), (0, w8 - 1, 1, 1), (h8 - 1, 0, 1, 1), (h8 - 1, w8 - 1, 1, 1),
            (h8 // 2, w8 // 2, 1, 1), (h8 // 2, 0, 1, w8), (0, w8 // 2, h8, 1)}
    if h8 >= 5 and w8 >= 5:
        wins.add((1, 2, h8 - 3, w8 - 4))
    return sorted(wins)


def plan_ref(H, W, y, x, bh, bw):
    """nic.h's rule, restated."""
    h8, w8 = -(-H // 8), -(-W // 8)
    ry0, ry1 = y // 8, (y + bh - 1) // 8 + 1
    rx0, rx1 = x // 8, (x + bw - 1) // 8 + 1
    r0, r1 = max(0, ry0 - HALO), min(h8, ry1 + HALO)
    c0, c1 = max(0, rx0 - HALO), min(w8, rx1 + HALO)
    return (r0, c0, r1 - r0, c1 - c0), (y - 8 * r0, x - 8 * c0)


def plan(H, W, y, x, bh, bw):
    win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
    rc = _lib.lib().nic_region_plan(H, W, y, x, bh, bw, win, off)
    return rc, tuple(win), tuple(off)


@pytest.mark.parametrize("H,W", [(37, 53), (64, 64), (9, 17)])
def test_region_plan_is_the_documented_rule(H, W):
    """Every box of the image (about one million, 4.3 million and seven thousand of them): one call of
    nic_region_plan each, against the restatement.  The restatement treats rows and columns apart, so
    its answers are tabulated once per (y, bh) and per (x, bw) and put together per box."""
    rows_of = {(y, bh): plan_ref(H, W, y, 0, bh, 1) for y in range(H) for bh in range(1, H - y + 1)}
    cols_of = {(x, bw): plan_ref(H, W, 0, x, 1, bw) for x in range(W) for bw in range(1, W - x + 1)}
    for (y, bh), (x, bw) in ((next(iter(rows_of)), next(iter(cols_of))), (max(rows_of), max(cols_of)), ((H // 3, H // 2), (W // 4, W // 2))):
        (r0, _, rows, _), (oy, _) = rows_of[y, bh]
        (_, c0, _, cols), (_, ox) = cols_of[x, bw]
        assert plan_ref(H, W, y, x, bh, bw) == ((r0, c0, rows, cols), (oy, ox))  # the tabulation is the restatement
    fn = _lib.lib().nic_region_plan
    out = (ctypes.c_int * 6)()  # win4, then off2
    off = ctypes.cast(ctypes.byref(out, 4 * ctypes.sizeof(ctypes.c_int)), ctypes.POINTER(ctypes.c_int))
    col_items = [(x, bw, c0, cols, ox) for (x, bw), ((_, c0, _, cols), (_, ox)) in cols_of.items()]
    checked = 0
    for (y, bh), ((r0, _, rows, _), (oy, _)) in rows_of.items():
        for x, bw, c0, cols, ox in col_items:
            if fn(H, W, y, x, bh, bw, out, off) != 0 or tuple(out) != (r0, c0, rows, cols, oy, ox):
                raise AssertionError(f"box {(y, x, bh, bw)}: rc and outputs {tuple(out)}, want {(r0, c0, rows, cols, oy, ox)}")
        checked += len(col_items)
    assert checked == (H * (H + 1) // 2) * (W * (W + 1) // 2)
    assert _lib.lib().nic_version() >= 700


def test_region_plan_refuses_bad_boxes():
    H, W = 37, 53
    for box in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -3, 4), (34, 0, 4, 4), (0, 50, 4, 4),
                (37, 0, 1, 1), (0, 53, 1, 1), (0, 0, 38, 53), (0, 0, 37, 54), (1, 0, 2 ** 31 - 1, 1), (0, 1, 1, 2 ** 31 - 1)):
        rc, _, _ = plan(H, W, *box)
        assert rc == _lib.NIC_ESHAPE, box
        assert "nic_region_plan" in _lib.last_error()
    assert plan(0, 8, 0, 0, 1, 1)[0] == _lib.NIC_ESHAPE and plan(8, -8, 0, 0, 1, 1)[0] == _lib.NIC_ESHAPE
    L = _lib.lib()
    win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
    assert L.nic_region_plan(H, W, 0, 0, 4, 4, None, off) == _lib.NIC_EINVAL
    assert L.nic_region_plan(H, W, 0, 0, 4, 4, win, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()
    assert plan(H, W, 36, 52, 1, 1) == (_lib.NIC_OK, (1, 3, 4, 4), (28, 28))  # hand-checked: rows 1..4 of 5, cols 3..6 of 7


def test_the_plan_is_exact_on_the_oracle(weights_spread):
    """The decoder's receptive field is within NIC_DECODE_HALO latent pixels: the oracle's decode of
    the planned window, cut at off2, is the crop of its decode of the whole latent, bit for bit."""
    h8, w8 = 13, 15
    H, W = 8 * h8, 8 * w8
    z = np.random.default_rng(7).integers(0, 256, (1, h8, w8, 96), dtype=np.uint8)
    whole = O.decode(weights_spread, z)
    assert whole.shape == (1, H, W, 3)
    boxes = [(13, 21, 30, 27),                                          # unaligned interior
             (0, 0, 9, 12), (0, W - 11, 7, 11), (H - 5, 0, 5, 9), (H - 10, W - 13, 10, 13),  # the four corners
             (40, 0, 8, W),                                             # a full row of latent pixels
             (51, 67, 1, 1)]                                            # one pixel
    for y, x, bh, bw in boxes:
        rc, (r0, c0, rows, cols), (oy, ox) = plan(H, W, y, x, bh, bw)
        assert rc == _lib.NIC_OK
        part = O.decode(weights_spread, np.ascontiguousarray(z[:, r0:r0 + rows, c0:c0 + cols]))
        np.testing.assert_array_equal(part[:, oy:oy + bh, ox:ox + bw], whole[:, y:y + bh, x:x + bw], str((y, x, bh, bw)))
    assert any(plan(H, W, *b)[1][2:] != (h8, w8) for b in boxes)  # the windows are real windows, not the latent


def segments(h8, w8, S, win):
    count = ctypes.c_int64(-1)
    rc = _lib.lib().nic_rans_window_segments(h8, w8, S, *win, ctypes.byref(count))
    return rc, count.value


@pytest.mark.parametrize("h8,w8", LATENTS)
def test_window_segments_counts_the_segments_of_the_window(h8, w8):
    for S in SEG_PIXELS:
        for win in windows_of(h8, w8):
            r0, c0, rows, cols = win
            want = len({((r0 + i) * w8 + c0 + j) // S for i in range(rows) for j in range(cols)})
            assert segments(h8, w8, S, win) == (_lib.NIC_OK, want), (S, win)
        assert segments(h8, w8, S, (0, 0, h8, w8))[1] == -(-h8 * w8 // S)  # the whole latent: every segment


def test_window_segments_refuses_bad_arguments():
    for win in ((-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, 0, 1), (0, 0, 1, 0), (12, 0, 2, 1), (0, 14, 1, 2), (13, 0, 1, 1),
                (1, 0, 2 ** 31 - 1, 1)):
        assert segments(13, 15, 32, win)[0] == _lib.NIC_ESHAPE, win
    assert segments(0, 15, 32, (0, 0, 1, 1))[0] == _lib.NIC_ESHAPE
    assert segments(13, 15, 0, (0, 0, 1, 1))[0] == _lib.NIC_ESHAPE
    assert segments(13, 15, 65536, (0, 0, 1, 1))[0] == _lib.NIC_ESHAPE
    assert _lib.lib().nic_rans_window_segments(13, 15, 32, 0, 0, 1, 1, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()


@pytest.mark.parametrize("name", ["nic_rans_decode_window", "nic_rans2_decode_window", "nic_rans3_decode_window"])
def test_decode_window_validates_without_a_gpu(name):
    # shape (the window included), empty batch, then NULL, all before any HIP call (the prior is
    # looked at last: NIC_ENOPRIOR needs a context, tests/test_gpu_region.py)
    f = getattr(_lib.lib(), name)
    big = 1 << 20
    assert f(None, None, big, None, 1, 4, 4, 0, 0, 4, 4, None, None, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error() and name + ":" in _lib.last_error()
    assert f(None, None, big, None, 1, 4, 0, 0, 0, 4, 4, None, None, None) == _lib.NIC_ESHAPE
    assert f(None, None, big, None, -1, 4, 4, 0, 0, 4, 4, None, None, None) == _lib.NIC_ESHAPE
    for win in ((-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, 0, 1), (0, 0, 1, 0), (3, 0, 2, 1), (0, 3, 1, 2), (4, 0, 1, 1)):
        assert f(None, None, big, None, 1, 4, 4, *win, None, None, None) == _lib.NIC_ESHAPE, win
        assert "window" in _lib.last_error()
        assert f(None, None, 0, None, 0, 4, 4, *win, None, None, None) == _lib.NIC_ESHAPE, win  # before the empty batch
    assert f(None, None, 0, None, 0, 4, 4, 1, 1, 2, 3, None, None, None) == _lib.NIC_OK  # empty batch
    assert f(None, None, big, None, 1, 4, 4, 3, 3, 1, 1, None, None, None) == _lib.NIC_EINVAL
