"""Device time of the resized-encode path beside what the library could do before it, in one process:
64 images of tools/region_batch_times.py's six frame sizes (its frames), each resized from its centred
box (codec.fit_boxes, "center") to 256 x 256 u8 and encoded:

  resample        the resize alone, sources resident on the device: one Codec.resample_pool launch over
                  the pool, against the baseline: per image F.interpolate(antialias=True) of the box, the
                  rounding to u8, and a stack
  host_to_u8      from the images in host memory to the (64, 256, 256, 3) u8 batch on the device:
                  Codec.resample_ragged (pack into one pinned pool, one upload, one launch), against a
                  per-image upload and the same torch ops
  host_to_files   from the images in host memory to the 64 version-2 .nic files in host memory:
                  Encoder.encode_resized + bitstream.nic_files, against the baseline's batch through
                  Codec.encode + bitstream.nic_files

hipEvents on the current stream, the median of `--iters` calls after `--warmup`, `--rounds` such medians
per form with the forms alternating (all reported).  Before timing, the two resizes are compared in fp32
(v / 255) with tools/crops_times.py's allowance: the float bound of tests/test_gpu_crops.py for each
side's sums, (4 + Ty + Tx) 2^-23 + 2^-23 |ref|, and torch's fp32 tap arguments, 2^-22 max(oh, ow).  The
largest use of the allowance is reported.  The host's image decoding is not part of any form: it is the
same on both sides and is timed once, per image with Pillow, for scale.

Output: one JSON line, also written to --out.  Needs the GPU and the built library."""
import argparse
import io
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = (256, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_compress_times.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from PIL import Image

    from neural_network_image_compression_amd import bitstream as B
    from neural_network_image_compression_amd import weights as W
    from neural_network_image_compression_amd.codec import Encoder, fit_boxes
    from neural_network_image_compression_amd.prior import Prior
    from tools.png_device_times import median_ms
    from tools.region_batch_times import FILES, SIZES

    pre = os.path.join(ROOT, "tests", "golden", "trained", "coef0.01_")
    enc = Encoder(0)
    enc.codec.set_weights(W.load(pre + "encoder", "encoder"))
    c = enc.codec
    d = os.path.join(ROOT, "data", "imagenet_patches_1k")
    names = B.list_dataset(d)[:FILES]
    x = np.stack([np.array(Image.open(os.path.join(d, fn)).convert("RGB")) for fn in names])
    with np.load(os.path.join(ROOT, "tests", "golden", "kodim21_full.npz"), allow_pickle=False) as g:
        full = g["x"][0]
    rng = np.random.default_rng(0)
    big = np.tile(full, (3, 3, 1))
    frames = []
    for i in range(FILES):  # region_batch_times' frames
        H, Wd = SIZES[i % len(SIZES)]
        if i % 2 == 0:
            y0, x0 = int(rng.integers(0, big.shape[0] - H + 1)), int(rng.integers(0, big.shape[1] - Wd + 1))
            frames.append(np.ascontiguousarray(big[y0:y0 + H, x0:x0 + Wd]))
        else:
            frames.append(np.ascontiguousarray(np.tile(x[i], (H // 128 + 1, Wd // 128 + 1, 1))[:H, :Wd]))
    boxes = fit_boxes([f.shape[:2] for f in frames], SIZE, "center")
    blist = boxes.tolist()
    z = enc.encode_resized(frames, SIZE, boxes)
    static = Prior.accumulator(c).add(z).build()
    c.set_prior(static)
    c.rans2_reserve(FILES, SIZE[0] // 8, SIZE[1] // 8)

    def torch_resize(t, box, dtype):
        oy, ox, bh, bw = box
        r = F.interpolate(t[oy:oy + bh, ox:ox + bw].permute(2, 0, 1)[None].float(), size=SIZE, mode="bilinear", align_corners=False,
                          antialias=True)
        if dtype == torch.uint8:
            return r.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
        return r / 255.0

    # agreement first, in fp32
    on_dev = [torch.from_numpy(f).cuda() for f in frames]
    ref = torch.cat([torch_resize(t, b, torch.float32) for t, b in zip(on_dev, blist)]).double()
    got = c.resample_ragged(frames, boxes, SIZE, dtype=torch.float32)
    taps = torch.tensor([[4 + math.ceil(2 * max(b[2] / SIZE[0], 1)) + 1 + math.ceil(2 * max(b[3] / SIZE[1], 1)) + 1] for b in blist],
                        dtype=torch.float64, device="cuda").view(FILES, 1, 1, 1)
    tol = 2 * taps * 2.0 ** -23 + 2.0 ** -22 * max(SIZE) + 2 * 2.0 ** -23 * ref.abs()
    use = float(((got.double() - ref).abs() / tol).max())
    assert use <= 1.0, use
    u8_new = c.resample_ragged(frames, boxes, SIZE, dtype=torch.uint8)
    u8_base = torch.cat([torch_resize(t, b, torch.uint8) for t, b in zip(on_dev, blist)]).contiguous()
    u8_differ = int((u8_new != u8_base).sum())  # roundings at a half: the two sums differ in their last bits

    pool, offsets, shapes = c.upload_pool(frames)
    table = np.empty((FILES, 8), np.int64)
    table[:, 0], table[:, 1:3], table[:, 3:7], table[:, 7] = offsets, shapes, boxes, np.arange(FILES)
    table = torch.from_numpy(table).cuda()
    result = torch.empty((FILES, *SIZE, 3), dtype=torch.uint8, device="cuda")
    assert torch.equal(c.resample_pool(pool, table, SIZE, torch.uint8, out=result), u8_new)

    def base_u8_host():
        return torch.cat([torch_resize(torch.from_numpy(f).cuda(), b, torch.uint8) for f, b in zip(frames, blist)]).contiguous()

    def new_files():
        return B.nic_files(c, enc.encode_resized(frames, SIZE, boxes), size=SIZE)

    def base_files():
        return B.nic_files(c, c.encode(base_u8_host()), size=SIZE)

    assert [B.nic2_inspect(f)[:5] for f in new_files()] == [(32, 32, B.NIC_SEG_PIXELS, *SIZE)] * FILES
    calls = {"resample_ms": lambda: c.resample_pool(pool, table, SIZE, torch.uint8, out=result),
             "resample_baseline_ms": lambda: torch.cat([torch_resize(t, b, torch.uint8) for t, b in zip(on_dev, blist)]),
             "host_to_u8_ms": lambda: c.resample_ragged(frames, boxes, SIZE, dtype=torch.uint8),
             "host_to_u8_baseline_ms": base_u8_host,
             "host_to_files_ms": new_files, "host_to_files_baseline_ms": base_files,
             "encode_and_files_ms": lambda: B.nic_files(c, c.encode(u8_new), size=SIZE)}
    times = {k: [] for k in calls}
    for _ in range(args.rounds):  # the forms alternate, so a drift of the machine shows in all
        for k, fn in calls.items():
            times[k].append(median_ms(torch, fn, args.warmup, args.iters))
    # the host's decoding of the same images from PNG, for scale: Pillow, one thread, per image
    pngs = [B.png_bytes(f, optimize=False) for f in frames]
    t0 = time.perf_counter()
    for p in pngs:
        np.array(Image.open(io.BytesIO(p)))
    pillow_ms = 1000.0 * (time.perf_counter() - t0)
    out = {"tool": "resize_compress_times", "iters": args.iters, "rounds": args.rounds, "files": FILES,
           "frame_sizes": [list(s) for s in SIZES], "size": list(SIZE), "mode": "center", "container": "nic version 2",
           "prior_id": f"{static.id:08x}", "source_bytes": int(sum(f.size for f in frames)), "box_bytes": int(sum(3 * b[2] * b[3] for b in blist)),
           "written_bytes": FILES * 3 * SIZE[0] * SIZE[1], "agreement_use_of_allowance": round(use, 4), "u8_differ": u8_differ,
           "u8_count": int(u8_new.numel()), "pillow_decode_one_thread_ms": round(pillow_ms, 2), **times}
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
