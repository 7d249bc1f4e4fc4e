"""CPU checks of the crops path's host side: nic_region_plan_window against the properties that make
windows of a given shape batchable and their cut exact, its exactness on the NumPy oracle for boxes of
different sizes planned to one shape, tests/resample_ref.py against torch's antialiased bilinear
interpolate, and the argument checks of nic_resample_boxes (no GPU calls here)."""
import ctypes

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from oracle import nic_oracle as O
from tests import resample_ref as RR
from tests.test_region_batch_format import boxes_of, fixed_count, plan_fixed
from tests.test_region_format import HALO, plan


def plan_window(H, W, y, x, bh, bw, rows_want, cols_want):
    win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
    rc = _lib.lib().nic_region_plan_window(H, W, y, x, bh, bw, rows_want, cols_want, win, off)
    return rc, tuple(win), tuple(off)


def need(len_):
    """nic.h's R: the most latent pixels len_ image pixels touch and the halo on both sides."""
    return (len_ + 6) // 8 + 1 + 2 * HALO


def test_window_plan_properties():
    """H, W in {8, 37, 64, 100, 203}, bh, bw in {1, 8, 9, 40}, every y, every seventh x and the last; the
    window shapes (R, C), (R + 1, C + 5) and one far above the latent."""
    sizes, lens = (8, 37, 64, 100, 203), (1, 8, 9, 40)
    checked = grown = 0
    for H in sizes:
        for W in sizes:
            h8, w8 = -(-H // 8), -(-W // 8)
            for bh in lens:
                for bw in lens:
                    R, C = need(bh), need(bw)
                    if bh > H or bw > W:
                        assert plan_window(H, W, 0, 0, bh, bw, R, C)[0] == _lib.NIC_ESHAPE
                        continue
                    for y in range(H - bh + 1):
                        for x in sorted(set(range(0, W - bw + 1, 7)) | {W - bw}):
                            box = (H, W, y, x, bh, bw)
                            rc1, (p0, q0, prows, pcols), _ = plan(*box)
                            assert rc1 == _lib.NIC_OK
                            for want in ((R, C), (R + 1, C + 5), (1000, 999)):
                                rc, (r0, c0, rows, cols), off = plan_window(*box, *want)
                                assert rc == _lib.NIC_OK, (box, want)
                                assert (rows, cols) == (min(h8, want[0]), min(w8, want[1])), (box, want)
                                assert 0 <= r0 and r0 + rows <= h8 and 0 <= c0 and c0 + cols <= w8, (box, want)
                                # it holds nic_region_plan's window
                                assert r0 <= p0 and p0 + prows <= r0 + rows and c0 <= q0 and q0 + pcols <= c0 + cols, (box, want)
                                # an edge is the frame's, or at least the halo beyond the latent pixels the box touches
                                assert r0 == 0 or r0 <= y // 8 - HALO, (box, want)
                                assert r0 + rows == h8 or r0 + rows >= (y + bh - 1) // 8 + 1 + HALO, (box, want)
                                assert c0 == 0 or c0 <= x // 8 - HALO, (box, want)
                                assert c0 + cols == w8 or c0 + cols >= (x + bw - 1) // 8 + 1 + HALO, (box, want)
                                # the rule itself
                                assert r0 == min(max(y // 8 - HALO, 0), h8 - rows) and c0 == min(max(x // 8 - HALO, 0), w8 - cols)
                                assert off == (y - 8 * r0, x - 8 * c0), (box, want)
                                assert off[0] >= 0 and off[0] + bh <= 8 * rows and off[1] >= 0 and off[1] + bw <= 8 * cols
                                if want == (R, C):
                                    assert (rc, (r0, c0, rows, cols), off) == plan_fixed(*box), box
                                else:
                                    grown += (rows, cols) != (fixed_count(bh, h8), fixed_count(bw, w8))
                                checked += 1
    assert checked > 300000 and grown > 10000
    assert _lib.lib().nic_version() >= 900


def test_window_plan_refusals():
    H, W = 100, 203
    for bh, bw in ((1, 1), (8, 9), (40, 40), (9, 2)):
        R, C = need(bh), need(bw)
        for want in ((R - 1, C), (R, C - 1), (0, C), (R, -5), (-(2 ** 31), C)):
            assert plan_window(H, W, 3, 5, bh, bw, *want)[0] == _lib.NIC_ESHAPE, (bh, bw, want)
            assert "nic_region_plan_window" in _lib.last_error()
        assert plan_window(H, W, 3, 5, bh, bw, R, C)[0] == _lib.NIC_OK
        assert plan_window(H, W, 3, 5, bh, bw, 2 ** 31 - 1, 2 ** 31 - 1)[:2] == (_lib.NIC_OK, (0, 0, 13, 26))
    # what the fixed plan refuses
    for box in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (97, 0, 4, 4), (0, 200, 4, 4), (1, 0, 2 ** 31 - 1, 1)):
        assert plan_fixed(H, W, *box)[0] == _lib.NIC_ESHAPE
        assert plan_window(H, W, *box, 50, 50)[0] == _lib.NIC_ESHAPE, box
    for H_, W_ in ((0, 8), (8, -8)):
        assert plan_window(H_, W_, 0, 0, 1, 1, 7, 7)[0] == _lib.NIC_ESHAPE
    L = _lib.lib()
    win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
    assert L.nic_region_plan_window(H, W, 0, 0, 4, 4, 8, 8, None, off) == _lib.NIC_EINVAL
    assert L.nic_region_plan_window(H, W, 0, 0, 4, 4, 8, 8, win, None) == _lib.NIC_EINVAL
    assert "NULL" in _lib.last_error()
    # hand-checked: the last pixel of a 203 x 203 image (26 x 26 latent pixels) in a 9 x 12 window
    assert plan_window(203, 203, 202, 202, 1, 1, 9, 12) == (_lib.NIC_OK, (17, 14, 9, 12), (66, 90))
    # the Python mirror
    from neural_network_image_compression_amd.codec import Codec

    assert Codec.region_plan_window(203, 203, (202, 202, 1, 1), (9, 12)) == ((17, 14, 9, 12), (66, 90))
    assert Codec.window_need(40, 24) == (12, 10) and Codec.window_need(1, 1) == (7, 7)
    with pytest.raises(ValueError, match="at least 7 x 7"):
        Codec.region_plan_window(203, 203, (202, 202, 1, 1), (6, 12))


@pytest.mark.parametrize("h8,w8", [(13, 15), (20, 9)])
def test_one_shape_for_boxes_of_three_sizes_is_exact_on_the_oracle(weights_spread, h8, w8):
    """Boxes of 40 x 24, 9 x 17 and 64 x 50 are planned to the largest need of the three, (15, 14); the
    oracle's decode of each window, cut at off2, is the crop of its decode of the whole latent."""
    H, W = 8 * h8, 8 * w8
    z = np.random.default_rng(12).integers(0, 256, (1, h8, w8, 96), dtype=np.uint8)
    whole = O.decode(weights_spread, z)
    boxes = [boxes_of(h8, w8)[5], boxes_of(h8, w8, 9, 17)[3], boxes_of(h8, w8, 64, 50)[1], boxes_of(h8, w8, 9, 17)[4]]
    want = (max(need(b[2]) for b in boxes), max(need(b[3]) for b in boxes))
    assert want == (15, 14)
    larger = 0
    for y, x, bh, bw in boxes:
        rc, (r0, c0, rows, cols), (oy, ox) = plan_window(H, W, y, x, bh, bw, *want)
        assert rc == _lib.NIC_OK and (rows, cols) == (min(h8, 15), min(w8, 14))
        larger += (rows, cols) != plan_fixed(H, W, y, x, bh, bw)[1][2:]
        part = O.decode(weights_spread, np.ascontiguousarray(z[:, r0:r0 + rows, c0:c0 + cols]))
        np.testing.assert_array_equal(part[:, oy:oy + bh, ox:ox + bw], whole[:, y:y + bh, x:x + bw], str((y, x, bh, bw)))
    assert larger >= 2


@pytest.mark.parametrize("shape,size", [((40, 24), (16, 16)), ((17, 33), (7, 5)), ((9, 9), (32, 24)), ((1, 1), (4, 4)),
                                        ((104, 120), (8, 8))])
def test_the_restatement_is_torch_interpolate(shape, size):
    """tests/resample_ref.py against F.interpolate(mode="bilinear", align_corners=False, antialias=True)
    on CPU float32 input, within torch's own fp32 rounding: the float bound of the GPU test at std 1."""
    torch = pytest.importorskip("torch")
    x = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 256, (*shape, 3), dtype=np.uint8)
    t = torch.from_numpy(x.astype(np.float32)).permute(2, 0, 1)[None]
    got = torch.nn.functional.interpolate(t, size=size, mode="bilinear", align_corners=False, antialias=True)[0]
    got = got.numpy().astype(np.float64) / 255.0
    for flip in (0, 1):
        ref, tol = RR.crop(x, (0, 0, *shape, flip), size, "float32")
        g = got[:, :, ::-1] if flip else got
        err = np.abs(g - ref)
        print(f"{shape} -> {size} flip {flip}: max |torch - ref| {err.max():.3e}, max of the bound's use {(err / tol).max():.3f}")
        assert ref.shape == (3, *size) and (err <= tol).all()
    if shape == (1, 1):
        assert (RR.resize(x, size)[0] == x[0, 0]).all()
    # equal sizes: one tap counts and the pixel comes through
    assert (RR.resize(x, shape)[0] == x).all()
    v, tol = RR.crop(x, (0, 0, *shape, 0), size, "uint8")
    assert v.shape == (*size, 3) and tol.min() >= 0.5 and RR.rounded_u8(v).dtype == np.uint8


def test_resample_boxes_validates_without_a_gpu():
    """Every argument check of nic_resample_boxes returns before a HIP call: the pointers here are not
    device memory."""
    L = _lib.lib()
    f = L.nic_resample_boxes
    three = (ctypes.c_float * 3)(1, 1, 1)
    a16 = 0x10000  # an aligned address that is never read
    ok = dict(ctx=a16, images=a16, n=1, Hs=8, Ws=8, table=a16, oh=4, ow=4, n_out=1, kind=0, scale=three, bias=three, out=a16)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["ctx"], a["images"], a["n"], a["Hs"], a["Ws"], a["table"], a["oh"], a["ow"], a["n_out"], a["kind"], a["scale"],
                 a["bias"], a["out"], None)

    for bad in (dict(n=-1), dict(n=65536), dict(n_out=0), dict(n_out=-3), dict(Hs=0), dict(Ws=0), dict(Hs=-8), dict(Hs=1 << 15, Ws=(1 << 14) + 1),
                dict(oh=0), dict(ow=0), dict(oh=16385), dict(ow=16385), dict(ow=-1), dict(n_out=1 << 12, oh=16384, ow=16384),
                dict(n_out=2 ** 31 - 1, oh=512, ow=1)):
        assert call(**bad) == _lib.NIC_ESHAPE, bad
        assert "nic_resample_boxes:" in _lib.last_error()
    for kind in (-1, 3, 7):
        assert call(kind=kind) == _lib.NIC_EINVAL and "out_kind" in _lib.last_error()
    # the shape and the kind come before the empty batch, the empty batch before NULL
    assert call(n=0, oh=0) == _lib.NIC_ESHAPE and call(n=0, kind=5) == _lib.NIC_EINVAL
    assert call(n=0, ctx=None, images=None, table=None, out=None, scale=None, bias=None) == _lib.NIC_OK
    assert call(n=65535, ctx=None) == _lib.NIC_EINVAL  # the largest batch passes the shape checks
    for null in ("ctx", "images", "table", "out", "scale", "bias"):
        assert call(**{null: None}) == _lib.NIC_EINVAL, null
        assert "NULL" in _lib.last_error()
    assert call(kind=1, bias=None) == _lib.NIC_EINVAL
    for bad in (dict(table=a16 + 2), dict(table=a16 + 1), dict(out=a16 + 8), dict(out=a16 + 4), dict(kind=2, out=a16 + 1)):
        assert call(**bad) == _lib.NIC_EINVAL and "aligned" in _lib.last_error(), bad
    assert (L.nic_version() >= 900)
