"""CPU checks of the resized-encode path's host side: codec.fit_boxes against the properties that define
it, by brute force; the argument checks of nic_resample_ragged (no GPU calls here); the pool packer."""
import ctypes

import numpy as np
import pytest

from neural_network_image_compression_amd import _lib
from neural_network_image_compression_amd import codec as C


def test_fit_boxes_properties():
    """64 output sizes (square, 4:3, 3:4, 16:9, extreme, 1 x n, n x 1 and random ones, sides 1..300), each
    with 5,000 random (H, W) of 1..300 and the (H, W) whose ratio agrees exactly: 320,000 and more cases.
    For every one the box lies inside the image, is centred to within one pixel, keeps one side whole,
    and no other integer length of the other side has a ratio nearer to the output's (compared exactly,
    cross-multiplied).  For a subset the nearest length is found by trying every one."""
    rng = np.random.default_rng(18)
    sizes = [(1, 1), (16, 16), (256, 256), (300, 300), (3, 4), (4, 3), (240, 300), (300, 225), (9, 16), (16, 9), (1, 300), (300, 1),
             (1, 7), (7, 1), (299, 300), (300, 299), (2, 3), (224, 224), (128, 96), (5, 300)]
    sizes += [tuple(int(v) for v in rng.integers(1, 301, 2)) for _ in range(44)]
    checked = whole = tried = 0
    for oh, ow in sizes:
        hw = rng.integers(1, 301, (5000, 2))
        k = np.arange(1, 300 // max(oh, ow) + 1)
        g = np.gcd(oh, ow)
        agree = np.stack([k * (oh // g), k * (ow // g)], axis=1) if k.size else np.zeros((0, 2), np.int64)
        agree = agree[(agree.max(axis=1) <= 300)] if agree.size else agree
        hw = np.concatenate([hw, agree, [[oh, ow]]]).astype(np.int64)
        H, W = hw[:, 0], hw[:, 1]
        for mode in ("center", "shorter"):
            b = C.fit_boxes(hw, (oh, ow), mode)
            assert b.shape == (len(hw), 4) and b.dtype == np.int64
            oy, ox, bh, bw = b.T
            assert (bh >= 1).all() and (bw >= 1).all() and (oy >= 0).all() and (ox >= 0).all()
            assert (oy + bh <= H).all() and (ox + bw <= W).all()
            # centred: twice the box's centre is twice the image's, or one less
            assert np.isin(2 * oy + bh - H, (0, -1)).all() and np.isin(2 * ox + bw - W, (0, -1)).all()
            # the largest: one side is the image's own, the one the ratio says
            wide = W * oh >= H * ow
            assert (bh[wide] == H[wide]).all() and (bw[~wide] == W[~wide]).all()
            # the nearest ratio, free side over whole side: |bw / H - ow / oh| = |bw oh - H ow| / (H oh) for a wide
            # image, |bh / W - oh / ow| = |bh ow - W oh| / (W ow) for a tall one; against both neighbours of the
            # free side (the distance is convex in it, so a local minimum is the minimum)
            miss = np.abs(bw * oh - bh * ow)
            for d in (-1, 1):
                other = bw[wide] + d
                ok = (other >= 1) & (other <= W[wide])
                assert (miss[wide][ok] <= np.abs(other * oh - bh[wide] * ow)[ok]).all()
                other = bh[~wide] + d
                ok = (other >= 1) & (other <= H[~wide])
                assert (miss[~wide][ok] <= np.abs(bw[~wide] * oh - other * ow)[ok]).all()
            same = W * oh == H * ow
            assert (b[same] == np.stack([0 * H, 0 * W, H, W], axis=1)[same]).all()
            whole += int(same.sum())
            checked += len(hw)
        # every length tried, for 200 of them
        b = C.fit_boxes(hw[:200], (oh, ow))
        for (h, w), (_, _, bh, bw) in zip(hw[:200].tolist(), b.tolist()):
            if w * oh >= h * ow:
                cand = np.arange(1, w + 1)
                assert abs(bw * oh - h * ow) == np.abs(cand * oh - h * ow).min()
            else:
                cand = np.arange(1, h + 1)
                assert abs(w * oh - bh * ow) == np.abs(w * oh - cand * ow).min()
            tried += 1
        s = C.fit_boxes(hw, (oh, ow), "stretch")
        assert (s == np.stack([0 * H, 0 * W, H, W], axis=1)).all()
    assert checked > 600000 and whole > 1000 and tried == 200 * len(sizes)
    # hand-checked: 480 x 640 to a square reads the middle 480 x 480; to 3 x 4 the whole; 2 x 1000 to 7 x 1 one column
    assert C.fit_boxes([(480, 640), (640, 480), (5, 5)], (256, 256)).tolist() == [[0, 80, 480, 480], [80, 0, 480, 480], [0, 0, 5, 5]]
    assert C.fit_boxes([(480, 640)], (3, 4)).tolist() == [[0, 0, 480, 640]]
    assert C.fit_boxes([(2, 1000)], (7, 1)).tolist() == [[0, 499, 2, 1]]
    assert C.fit_boxes([], (4, 4)).shape == (0, 4)
    for bad in (dict(shapes=[(0, 4)], size=(4, 4)), dict(shapes=[(4, 4)], size=(0, 4)), dict(shapes=[(4, 4)], size=4),
                dict(shapes=[(4, 4)], size=(4, 4), mode="fill")):
        with pytest.raises(ValueError):
            C.fit_boxes(**bad)


def test_resample_ragged_validates_without_a_gpu():
    """Every argument check of nic_resample_ragged returns before a HIP call: the pointers here are not
    device memory."""
    L = _lib.lib()
    f = L.nic_resample_ragged
    three = (ctypes.c_float * 3)(1, 1, 1)
    a16 = 0x10000  # an aligned address that is never read
    ok = dict(ctx=a16, pool=a16, pool_bytes=192, n=1, table=a16, oh=4, ow=4, n_out=1, kind=0, scale=three, bias=three, out=a16)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["ctx"], a["pool"], a["pool_bytes"], a["n"], a["table"], a["oh"], a["ow"], a["n_out"], a["kind"], a["scale"],
                 a["bias"], a["out"], None)

    for bad in (dict(n=-1), dict(n=65536), dict(pool_bytes=-1), dict(pool_bytes=-(2 ** 63)), dict(n_out=0), dict(n_out=-3),
                dict(oh=0), dict(ow=0), dict(oh=16385), dict(ow=16385), dict(ow=-1), dict(n_out=1 << 12, oh=16384, ow=16384),
                dict(n_out=2 ** 31 - 1, oh=512, ow=1)):
        assert call(**bad) == _lib.NIC_ESHAPE, bad
        assert "nic_resample_ragged:" in _lib.last_error()
    for kind in (-1, 3, 7):
        assert call(kind=kind) == _lib.NIC_EINVAL and "out_kind" in _lib.last_error()
    # the shape and the kind come before the empty batch, the empty batch before NULL
    assert call(n=0, oh=0) == _lib.NIC_ESHAPE and call(n=0, kind=5) == _lib.NIC_EINVAL and call(n=0, pool_bytes=-4) == _lib.NIC_ESHAPE
    assert call(n=0, ctx=None, pool=None, table=None, out=None, scale=None, bias=None) == _lib.NIC_OK
    assert call(n=65535, pool_bytes=2 ** 62, ctx=None) == _lib.NIC_EINVAL  # the largest batch and pool pass the shape checks
    for null in ("ctx", "pool", "table", "out", "scale", "bias"):
        assert call(**{null: None}) == _lib.NIC_EINVAL, null
        assert "NULL" in _lib.last_error()
    assert call(kind=1, bias=None) == _lib.NIC_EINVAL
    for bad in (dict(pool=a16 + 1), dict(pool=a16 + 2), dict(table=a16 + 4), dict(table=a16 + 1), dict(out=a16 + 8), dict(out=a16 + 4),
                dict(kind=2, out=a16 + 1)):
        assert call(**bad) == _lib.NIC_EINVAL and "aligned" in _lib.last_error(), bad
    assert L.nic_version() >= 1000
    assert "nic_resample_ragged" in _lib.header_symbols()


def test_the_packer():
    rng = np.random.default_rng(19)
    shapes = [(1, 1), (1, 7), (5, 1), (3, 5), (37, 53), (64, 48), (50, 67), (16, 16)]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    images[4] = np.ascontiguousarray(images[4][::-1])[::-1]  # a view with negative strides: packed by value
    pool, offsets = C.pack_images(images)
    want_offsets, total = C.pool_layout(shapes)
    assert offsets == want_offsets and pool.dtype == np.uint8 and pool.shape == (total,)
    assert offsets[0] == 0 and all(o % C.POOL_ALIGN == 0 for o in offsets) and C.POOL_ALIGN == 16
    # as close as the alignment allows, in order, and the pool ends on the last image's last byte
    for (h, w), o, nxt in zip(shapes, offsets, offsets[1:] + [None]):
        end = o + 3 * h * w
        assert nxt is None and end == total or end <= nxt < end + C.POOL_ALIGN
    # a pool rebuilt from the table equals the inputs: tight rows, pitch 3 W
    for a, o in zip(images, offsets):
        h, w, _ = a.shape
        np.testing.assert_array_equal(pool[o:o + 3 * h * w].reshape(h, w, 3), a)
        np.testing.assert_array_equal(pool[o + 3 * w * (h - 1):o + 3 * w * h], a[h - 1].reshape(-1))
    # into a buffer of the caller's: the padding keeps what it held
    mine = np.full(total + 5, 0xEE, np.uint8)
    got, _ = C.pack_images(images, mine)
    assert got is mine and (mine[total:] == 0xEE).all() and (mine[3:16] == 0xEE).all()
    np.testing.assert_array_equal(mine[offsets[6]:offsets[6] + images[6].size], images[6].reshape(-1))
    for bad, text in (([np.zeros((4, 4, 4), np.uint8)], "image 0"), ([images[0], np.zeros((4, 4, 3), np.float32)], "image 1"),
                      ([np.zeros((0, 4, 3), np.uint8)], "image 0"), ([np.zeros((4, 4), np.uint8)], "image 0")):
        with pytest.raises(ValueError, match=text):
            C.pack_images(bad)
    with pytest.raises(ValueError, match="pool"):
        C.pack_images(images, np.zeros(total - 1, np.uint8))
    assert C.pool_layout([]) == ([], 0)
