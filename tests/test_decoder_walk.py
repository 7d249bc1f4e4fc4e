"""tests/decoder_walk.py, the restated launch splits of the decoder's persistent kernels: the
cross-over batches test_decode_tile_counts_* (tests/test_gpu_parity.py) run on a 256-CU device,
worked out by hand from launch_dconv1_all and launch_ws, and the splits' own invariants."""
import pytest

from tests import decoder_walk as W


def test_crossovers_on_256_cus():
    """(n, 1, 1) latents, one dconv1 tile and one dconv7 tile per plane.  dconv1: by = min(n, 85),
    bc = min(2 n, 171); dconv7: 171 of 512 blocks for Y, 341 for CbCr (512 / 3 = 170.67 and
    341.33, each rounded after + 1/2)."""
    x = {(kernel, group, k): n for kernel, group, k, n in W.crossovers(256, 1, 1, 4)}
    assert x[("dconv1", "Y", 1)] == 85 and x[("dconv1", "CbCr", 1)] == 85
    assert x[("dconv1", "Y", 2)] == 170 and x[("dconv7", "CbCr", 1)] == 170
    assert x[("dconv7", "Y", 1)] == 171 and x[("dconv1", "CbCr", 2)] == 171
    assert x[("dconv1", "Y", 3)] == 255 and x[("dconv1", "Y", 4)] == 340
    assert x[("dconv7", "CbCr", 2)] == 341 and x[("dconv7", "Y", 2)] == 342 and x[("dconv7", "Y", 3)] == 513
    got = W.crossover_batches(256, 1, 1, 3)
    for n in (85, 170, 171, 255, 341, 342, 513):
        assert n in got and n + 1 in got, (n, got)
    # and the CbCr groups' 3 -> 4: 3 * 171 = 513 < 2 * 257 (dconv1), 3 * 341 = 1023 < 2 * 512 (dconv7)
    assert got == [85, 86, 170, 171, 172, 255, 256, 257, 341, 342, 343, 511, 512, 513, 514]


def test_partial_tile_crossovers_on_256_cus():
    """(n, 1, 9) latents: 2 dconv1 tiles and 3 dconv7 tiles per plane."""
    got = W.crossover_batches(256, 1, 9, 2)
    for n in (42, 57, 85, 114):
        assert n in got and n + 1 in got, (n, got)
    assert got == [42, 43, 56, 57, 58, 85, 86, 113, 114, 115]


@pytest.mark.parametrize("cus", [8, 64, 104, 256, 304])
@pytest.mark.parametrize("shape,kmax", [((1, 1), 4), ((1, 9), 3), ((3, 8), 2), ((5, 24), 2)])
def test_every_crossover_is_one(cus, shape, kmax):
    """Each listed n has the claimed maximum, n + 1 has one more (whole planes arrive at once, so
    with several tiles per plane the step may be larger, never smaller), and the batches hold both."""
    h8, w8 = shape
    xs = W.crossovers(cus, h8, w8, kmax)
    if shape == (1, 1):  # one tile per plane: every group passes through every k
        assert {(kernel, group, k) for kernel, group, k, _ in xs} == {
            (kernel, group, k) for kernel in W.KERNELS for group in W.GROUPS for k in range(1, kmax + 1)}
    batches = W.crossover_batches(cus, h8, w8, kmax)
    assert batches == sorted(set(batches))
    for kernel, group, k, n in xs:
        gi = W.GROUPS.index(group)
        assert W.max_tiles(kernel, gi, cus, n, h8, w8) == k, (kernel, group, k, n)
        after = W.max_tiles(kernel, gi, cus, n + 1, h8, w8)
        assert after > k and (after == k + 1 or h8 * w8 > 1), (kernel, group, k, n, after)
        assert n in batches and n + 1 in batches
        # the maximum never falls as the batch grows, so `largest n` is what the upward scan found
        assert all(W.max_tiles(kernel, gi, cus, m, h8, w8) > k for m in range(n + 1, n + 40))


@pytest.mark.parametrize("cus", [8, 64, 104, 256, 304])
def test_no_empty_block_and_every_tile_walked(cus):
    """No group ever gets a block without a tile (the kernels' ntile = 0 path is never launched),
    the blocks' tile counts sum to the group's tiles, the grids stay inside what the device holds
    (dconv1: one block per CU; dconv7: two), and the pair's grid has 4 rows per block at least."""
    for h8, w8 in [(1, 1), (1, 9), (3, 8), (5, 24), (40, 2)]:
        for n in list(range(1, 48)) + [85, 86, 171, 172, 343, 514, 1000]:
            for kernel, groups in W.KERNELS.items():
                tiles, blocks = groups(cus, n, h8, w8)
                assert sum(blocks) <= (cus if kernel == "dconv1" else 2 * cus + 1), (kernel, cus, n, blocks)
                for t, b in zip(tiles, blocks):
                    walk = W.tiles_per_block(t, b)
                    assert len(walk) == b >= 1 and min(walk) >= 1 and sum(walk) == t, (kernel, cus, n, h8, w8)
                    assert max(walk) - min(walk) <= 1
            rows, grid = W.pair_grid(cus, n, h8, w8)
            assert rows == 3 * n * 2 * h8 and 1 <= grid <= cus and (grid == cus or 4 * grid >= rows > 4 * (grid - 1))


def test_tiles_per_block():
    assert W.tiles_per_block(5, 2) == [3, 2]
    assert W.tiles_per_block(3, 3) == [1, 1, 1]
    assert W.tiles_per_block(2, 3) == [1, 1, 0]  # the kernels' bi >= ntot; the launches never make one
    assert W.pair_strips(64) == 1 and W.pair_strips(66) == 0 and W.pair_strips(118) == 2 and W.pair_strips(176) == 3
