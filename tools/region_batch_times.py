"""Device time of batched region decode beside the per-file loop, in one process: a 224x224 box at a
seeded random position out of each of 64 .nic files of six different frame sizes (288x352 to
768x1024; even files cropped from a tiling of kodim21, odd files tiled from one patch each of
data/imagenet_patches_1k), with the trained coef-0.01 codec, for .nic versions 2 and 3 (priors fitted
on the first 200 files, sorted, of data/imagenet_patches_1k, as tools/region_decode_times.py),
seg_pixels 32:

  pixels       Decoder.decode_regions(files, boxes), one call, against 64 calls of
               Decoder.decode_region([file], box): from the files' bytes in host memory (host checks,
               upload of the whole files, window entropy decode, the decoder on the windows, the cut)
  pixels_dev   the device part of both alone, files resident on the device: one
               Codec.rans*_decode_windows_status + Codec.decode + Codec.cut_boxes against 64 times
               Codec.rans*_decode_window_status + Codec.decode + slice
  entropy      the entropy stage of both alone, files resident on the device

hipEvents on the current stream, the median of `--iters` calls after `--warmup`, `--rounds` such
medians per form with the two forms alternating (all reported); workspaces are reserved first.
The batch's result is first checked equal to the loop's.

Output: one JSON line.  Needs the GPU and the built library."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((288, 352), (384, 512), (512, 768), (300, 420), (768, 1024), (480, 640))
BOX = 224
FILES = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from PIL import Image

    from neural_network_image_compression_amd import bitstream as B
    from neural_network_image_compression_amd import weights as W
    from neural_network_image_compression_amd.codec import Codec, Decoder
    from neural_network_image_compression_amd.prior import ContextPrior, Prior
    from tools.png_device_times import median_ms

    pre = os.path.join(ROOT, "tests", "golden", "trained", "coef0.01_")
    c = Codec(0)
    c.set_weights(W.load(pre + "encoder", "encoder"))
    c.set_weights(W.load(pre + "decoder", "decoder"))
    dec = Decoder(codec=c)
    d = os.path.join(ROOT, "data", "imagenet_patches_1k")
    names = B.list_dataset(d)[:200]
    x = np.stack([np.array(Image.open(os.path.join(d, fn)).convert("RGB")) for fn in names])
    z = torch.cat([c.encode(torch.from_numpy(x[i:i + 100]).cuda()) for i in range(0, 200, 100)])
    static = Prior.accumulator(c).add(z).build()
    cprior = ContextPrior.accumulator(c, static).add(z).build()
    with np.load(os.path.join(ROOT, "tests", "golden", "kodim21_full.npz"), allow_pickle=False) as g:
        full = g["x"][0]
    rng = np.random.default_rng(0)
    big = np.tile(full, (3, 3, 1))
    frames, boxes = [], []
    for i in range(FILES):
        H, Wd = SIZES[i % len(SIZES)]
        if i % 2 == 0:
            y0, x0 = int(rng.integers(0, big.shape[0] - H + 1)), int(rng.integers(0, big.shape[1] - Wd + 1))
            frames.append(np.ascontiguousarray(big[y0:y0 + H, x0:x0 + Wd]))
        else:
            frames.append(np.ascontiguousarray(np.tile(x[i], (H // 128 + 1, Wd // 128 + 1, 1))[:H, :Wd]))
        boxes.append((int(rng.integers(0, H - BOX + 1)), int(rng.integers(0, Wd - BOX + 1)), BOX, BOX))
    lats = [c.encode(torch.from_numpy(f[None]).cuda()) for f in frames]
    out = {"tool": "region_batch_times", "iters": args.iters, "rounds": args.rounds, "prior_id": f"{static.id:08x}",
           "context_prior_id": f"{cprior.id:08x}", "fitted_on": "imagenet_patches_1k[0:200]", "files": FILES,
           "frame_sizes": [list(s) for s in SIZES], "box": [BOX, BOX], "seg_pixels": B.NIC_SEG_PIXELS}
    c.reserve(FILES, 280, 280)  # the batch: 64 windows of 35 x 35 latent pixels
    c.reserve(1, *max(SIZES))
    for ver in (2, 3):
        c.set_prior(static if ver == 2 else None)  # nic_files writes version 3 when a context prior is set
        c.set_context_prior(cprior if ver == 3 else None)
        files = [B.nic_files(c, lat, size=f.shape[:2])[0] for lat, f in zip(lats, frames)]
        assert all(f[4] == ver for f in files)
        (c.rans2_reserve if ver == 2 else c.rans3_reserve)(FILES, 96, 128)
        win_status = c.rans2_decode_window_status if ver == 2 else c.rans3_decode_window_status
        wins_status = c.rans2_decode_windows_status if ver == 2 else c.rans3_decode_windows_status
        # the loop's plans and resident files, one per call; the batch's table and resident files, one upload
        singles = []
        for f, lat, frame, box in zip(files, lats, frames, boxes):
            win, (oy, ox) = Codec.region_plan(frame.shape[0], frame.shape[1], box)
            singles.append((*B._upload_files(c, [f]), lat.shape[1], lat.shape[2], win, oy, ox))
        plans = [Codec.region_plan_fixed(frame.shape[0], frame.shape[1], box) for frame, box in zip(frames, boxes)]
        shape = plans[0][0][2:]
        assert all(p[0][2:] == shape for p in plans)  # every frame holds the fixed window: one group
        table = torch.tensor([(lat.shape[1], lat.shape[2], p[0][0], p[0][1]) for lat, p in zip(lats, plans)],
                             dtype=torch.int32, device="cuda")
        offs = torch.tensor([p[1] for p in plans], dtype=torch.int32, device="cuda")
        max_pixels = max(lat.shape[1] * lat.shape[2] for lat in lats)
        buf, sizes = B._upload_files(c, files)

        def batch_entropy():
            return wins_status(buf, sizes, table, shape, max_pixels=max_pixels)[0]

        def loop_entropy():
            return [win_status(b, s, h8, w8, win)[0] for b, s, h8, w8, win, _, _ in singles]

        def batch_dev():
            return c.cut_boxes(c.decode(batch_entropy()), offs, BOX, BOX)

        def loop_dev():
            return [c.decode(win_status(b, s, h8, w8, win)[0])[:, oy:oy + BOX, ox:ox + BOX].contiguous()
                    for b, s, h8, w8, win, oy, ox in singles]

        def batch_host():
            return dec.decode_regions(files, boxes)

        def loop_host():
            return [dec.decode_region([f], box) for f, box in zip(files, boxes)]

        ref = torch.cat(loop_host())
        assert torch.equal(batch_host(), ref) and torch.equal(batch_dev(), ref) and torch.equal(torch.cat(loop_dev()), ref)
        for lat, frame, box, r in zip(lats[:6], frames, boxes, ref):  # and the loop is the crop of the whole decode
            assert torch.equal(c.decode(lat)[0, box[0]:box[0] + BOX, box[1]:box[1] + BOX], r)
        calls = {"entropy_batch_ms": batch_entropy, "entropy_loop_ms": loop_entropy, "pixels_dev_batch_ms": batch_dev,
                 "pixels_dev_loop_ms": loop_dev, "pixels_batch_ms": batch_host, "pixels_loop_ms": loop_host}
        times = {k: [] for k in calls}
        for _ in range(args.rounds):  # the forms alternate, so a drift of the box shows in both
            for k, fn in calls.items():
                times[k].append(median_ms(torch, fn, args.warmup, args.iters))
        out[f"v{ver}"] = {"file_bytes": [min(map(len, files)), max(map(len, files))], "window": list(shape),
                          "equal_to_loop": True, **times}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
