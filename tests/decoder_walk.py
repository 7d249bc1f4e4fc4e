"""The launch splits of the decoder's persistent f16x3 kernels, restated from
neural_network_image_compression_amd/csrc/nic_kernels.hip in plain Python (no torch, no numpy), for
tests/test_decoder_walk.py (CPU) and test_decode_tile_counts_* in tests/test_gpu_parity.py.

What a block of these kernels does depends on how many tiles it walks: dconv1_all_kernel runs its
tiles in pairs with an odd tail, prefetches codes two tiles ahead and alternates two LDS halo
buffers by tile parity (d1all_wave); conv_ws_kernel's dconv7 runs four ws_body phases over the
block's tiles, each storing tile i - 1's projection during tile i.  The GPU tests therefore decode
batches that land on every cross-over of the maximum tiles per block, and they take those batch
sizes from here.  Every function is given `cus`, the device's compute units (device_cus()), the
batch n and the latent's h8 x w8; a latent plane is h8 x w8 for dconv1 and 2 h8 x 2 w8 for the
dconv5+dconv6 pair and for dconv7 (decode_pass, csrc/nic_capi.hip).

A change to launch_dconv1_all's split ((target + 1) / 3 blocks for Y, the rest for CbCr), to
launch_ws's target (2 * device_cus()) or its rounded split, or to the strided walk (block bi of nb
takes tiles bi, bi + nb, ..) moves these cross-overs: restate it here, and the GPU tests'
batches follow.  With a restatement that no longer matches the device the batches would merely
stop landing on the cross-overs, so the GPU tests compare dconv1_groups, dconv7_groups and
pair_grid with the grids the launches' own split functions give for every batch
(Codec.decode_launch_info, nic_decode_launch_info), and the CPU test pins the figures for 256 CUs.
"""

GROUPS = ("Y", "CbCr")  # model group 0: the n Y planes, 1: the 2 n Cb and Cr planes


def _cdiv(a, b):
    return -(-a // b)


def dconv1_groups(cus, n, h8, w8):
    """launch_dconv1_all: ((tiles Y, tiles CbCr), (by, bc)) for 8 x 8 tiles of the h8 x w8 codes."""
    per_plane = _cdiv(h8, 8) * _cdiv(w8, 8)            # a.tiles_y * a.tiles_x
    ty, tc = n * per_plane, 2 * n * per_plane          # ty, tc
    target = cus                                       # target = device_cus()
    by = max(1, min(ty, (target + 1) // 3))            # by
    bc = max(1, min(tc, target - by))                  # bc
    return (ty, tc), (by, bc)


def dconv7_groups(cus, n, h8, w8):
    """launch_ws<64, 64, 8, 8, false, true, true> (launch_dconv7_proj_x3): ((tiles Y, tiles CbCr),
    (blocks Y, blocks CbCr)) for 8 x 8 tiles of the 2 h8 x 2 w8 input plane."""
    per_plane = _cdiv(2 * h8, 8) * _cdiv(2 * w8, 8)    # a.tiles_y * a.tiles_x, TH = TW = 8
    work = (n * per_plane, 2 * n * per_plane)          # work[gi] = (gi & 1 ? P - nimg : nimg) * per_plane
    total = work[0] + work[1]
    target = 2 * cus                                   # target = 2 * device_cus()
    blocks = []
    for gi in range(2):
        tiles = work[gi]                               # tiles: the same product as work[gi]
        b = (work[gi] * target + total // 2) // total  # rounded share of the target
        b = 1 if b < 1 else tiles if b > tiles else b  # clipped to [1, tiles]
        blocks.append(b)
    return work, tuple(blocks)


def pair_strips(w):
    """k3pair_strips: strips of a plane of w columns (0: the fused pair does not take it)."""
    if w <= 64:                                        # K3P_MAX_W
        return 1
    s = _cdiv(w, 62)                                   # K3P_SW
    return s if 10 * s * 64 <= 11 * w else 0


def pair_grid(cus, n, h8, w8):
    """launch_k3pair_x3: (rows of the stream of all planes' rows, grid), plane 2 h8 x 2 w8."""
    rows = 3 * n * pair_strips(2 * w8) * 2 * h8        # rows = a.P * a.tiles_x * a.H
    grid = max(1, min(_cdiv(rows, 4), cus))            # sr = 4 rows per block at least, one block per CU
    return rows, grid


def tiles_per_block(tiles, nb):
    """ntile of each block bi of a group of nb (d1all_wave, ws_body): block bi walks tiles bi,
    bi + nb, .. of its group's `tiles`, ntile = ceil((tiles - bi) / nb), 0 past the last tile."""
    return [_cdiv(tiles - bi, nb) if bi < tiles else 0 for bi in range(nb)]


KERNELS = {"dconv1": dconv1_groups, "dconv7": dconv7_groups}


def max_tiles(kernel, group, cus, n, h8, w8):
    """The most tiles one block of `kernel`'s model group `group` (0: Y, 1: CbCr) walks."""
    tiles, blocks = KERNELS[kernel](cus, n, h8, w8)
    return max(tiles_per_block(tiles[group], blocks[group]))


def crossovers(cus, h8, w8, kmax):
    """[(kernel, group name, k, n)]: for each (kernel, model group) and k = 1..kmax the largest
    batch n whose maximum tiles per block is k, found by scanning n upward until the maximum passes
    kmax (it never falls as n grows: the blocks of a group saturate, the tiles keep growing).  A k
    that no n gives (many tiles per plane: the maximum steps over it) has no entry."""
    out = []
    for kernel in KERNELS:
        for group, name in enumerate(GROUPS):
            last = {}
            n = 1
            while True:
                k = max_tiles(kernel, group, cus, n, h8, w8)
                if k > kmax:
                    break
                last[k] = n
                n += 1
            out += [(kernel, name, k, last[k]) for k in sorted(last)]
    return out


def crossover_batches(cus, h8, w8, kmax):
    """The batch sizes either side of every cross-over of crossovers(): n and n + 1, sorted."""
    return sorted({m for _, _, _, n in crossovers(cus, h8, w8, kmax) for m in (n, n + 1)})


def describe(cus, n, h8, w8):
    """One line for a failure message: each kernel's blocks per group and the most tiles a block
    walks, and the pair's rows and grid."""
    parts = []
    for kernel, groups in KERNELS.items():
        tiles, blocks = groups(cus, n, h8, w8)
        walk = [max(tiles_per_block(t, b)) for t, b in zip(tiles, blocks)]
        parts.append(f"{kernel} blocks Y {blocks[0]} CbCr {blocks[1]}, max tiles per block Y {walk[0]} CbCr {walk[1]}")
    rows, grid = pair_grid(cus, n, h8, w8)
    parts.append(f"pair {rows} rows on {grid} blocks")
    return "; ".join(parts)
