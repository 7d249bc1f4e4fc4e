"""Device time of Decoder.decode_crops beside what the library could do before it, in one process: one
box per file, drawn the way RandomResizedCrop draws (8-100 % of the image's area, aspect ratio 3/4 to
4/3, seed 0), out of tools/region_batch_times.py's 64 .nic files of six frame sizes, with its codec and
priors, resized to 224 x 224 f16 NCHW with the ImageNet mean and std, every second box mirrored:

  pixels       from the files' bytes in host memory: Decoder.decode_crops with bucket=None and with
               bucket=8, against the baseline: per file Decoder.decode_region, then
               F.interpolate(antialias=True), the flip, the normalisation and the cast on the device,
               then a stack
  pixels_dev   the device part of each alone, files resident on the device: per group one
               Codec.rans*_decode_windows_status + Codec.decode + Codec.resample_boxes; the baseline's
               per-file Codec.rans*_decode_window_status + Codec.decode + slice and the same torch ops
  resample     Codec.resample_boxes alone on the bucket=None groups' reconstructions, with the bytes it
               reads (the boxes) and writes

hipEvents on the current stream, the median of `--iters` calls after `--warmup`, `--rounds` such
medians per form with the forms alternating (all reported).  Before timing, decode_crops (fp32) is
checked against the baseline (fp32).  The allowance has two parts.  One is the float bound of
tests/test_gpu_crops.py for each side's sums, (4 + Ty + Tx) 2^-23 / std + 2^-23 |ref| with Ty, Tx the
tap counts ceil(2 max(in / out, 1)) + 1.  The other is torch's alone: it evaluates a tap's centre
c = s (i + 0.5) and the weight's argument in fp32, two roundings of a number as large as c, so every
argument of output i is shifted by up to 2^-22 c / support <= 2^-22 (i + 0.5), and a shift d of all
arguments moves the output by at most d times the range of the pixels, 1 in 0..1 units: up to
2^-22 max(oh, ow) / std at the last outputs (on a CPU, torch's fp32 result is 12 times the float bound
from the float64 restatement for 150x180 -> 224x224; the kernel, whose tap geometry is integer, a
tenth).  The largest use of the allowance is reported.

Output: one JSON line.  Needs the GPU and the built library."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = (224, 224)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def draw_box(rng, H, W):
    """torchvision's RandomResizedCrop.get_params with scale (0.08, 1) and ratio (3/4, 4/3)."""
    for _ in range(10):
        area = H * W * rng.uniform(0.08, 1.0)
        ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        w, h = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
    return 0, 0, H, W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from PIL import Image

    from neural_network_image_compression_amd import bitstream as B
    from neural_network_image_compression_amd import weights as W
    from neural_network_image_compression_amd.codec import Codec, Decoder
    from neural_network_image_compression_amd.prior import ContextPrior, Prior
    from tools.png_device_times import median_ms
    from tools.region_batch_times import FILES, SIZES

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
    frames = []
    for i in range(FILES):  # region_batch_times' frames
        H, Wd = SIZES[i % len(SIZES)]
        if i % 2 == 0:
            y0, x0 = int(rng.integers(0, big.shape[0] - H + 1)), int(rng.integers(0, big.shape[1] - Wd + 1))
            frames.append(np.ascontiguousarray(big[y0:y0 + H, x0:x0 + Wd]))
        else:
            frames.append(np.ascontiguousarray(np.tile(x[i], (H // 128 + 1, Wd // 128 + 1, 1))[:H, :Wd]))
    rng = np.random.default_rng(0)
    boxes = [draw_box(rng, *f.shape[:2]) for f in frames]
    flips = [i % 2 for i in range(FILES)]
    lats = [c.encode(torch.from_numpy(f[None]).cuda()) for f in frames]
    mean_t = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    out_bytes = FILES * 3 * SIZE[0] * SIZE[1] * 2
    box_bytes = sum(3 * b[2] * b[3] for b in boxes)
    out = {"tool": "crops_times", "iters": args.iters, "rounds": args.rounds, "prior_id": f"{static.id:08x}",
           "context_prior_id": f"{cprior.id:08x}", "fitted_on": "imagenet_patches_1k[0:200]", "files": FILES,
           "frame_sizes": [list(s) for s in SIZES], "size": list(SIZE), "dtype": "float16", "seg_pixels": B.NIC_SEG_PIXELS,
           "box_area_fraction": [round(min(b[2] * b[3] / (f.shape[0] * f.shape[1]) for b, f in zip(boxes, frames)), 3),
                                 round(max(b[2] * b[3] / (f.shape[0] * f.shape[1]) for b, f in zip(boxes, frames)), 3)],
           "resample_bytes": {"read_boxes": box_bytes, "written": out_bytes}}

    def torch_tail(cut, flip, dtype):
        t = F.interpolate(cut.permute(0, 3, 1, 2).float(), size=SIZE, mode="bilinear", align_corners=False, antialias=True)
        if flip:
            t = t.flip(3)
        return ((t / 255.0 - mean_t) / std_t).to(dtype)

    for ver in (2, 3):
        c.set_prior(static if ver == 2 else None)  # nic_files writes version 3 when a context prior is set
        c.set_context_prior(cprior if ver == 3 else None)
        files = [B.nic_files(c, lat, size=f.shape[:2])[0] for lat, f in zip(lats, frames)]
        assert all(f[4] == ver for f in files)
        (c.rans2_reserve if ver == 2 else c.rans3_reserve)(FILES, 96, 128)
        win_status = c.rans2_decode_window_status if ver == 2 else c.rans3_decode_window_status
        wins_status = c.rans2_decode_windows_status if ver == 2 else c.rans3_decode_windows_status
        singles = []
        for f, lat, frame, box in zip(files, lats, frames, boxes):
            win, (oy, ox) = Codec.region_plan(frame.shape[0], frame.shape[1], box)
            singles.append((*B._upload_files(c, [f]), lat.shape[1], lat.shape[2], win, oy, ox, box[2], box[3]))
        max_pixels = max(lat.shape[1] * lat.shape[2] for lat in lats)

        def resident(bucket):
            """Per group: the files on the device, the window table, the shape, the resample table."""
            _, _, groups = B._window_groups_any(c, files, boxes, bucket, "crops_times", [f"file {i}" for i in range(FILES)])
            res = []
            for shape, members in groups.items():
                idx = [m[0] for m in members]
                buf, sizes = B._upload_files(c, [files[i] for i in idx])
                tab = torch.tensor([m[1] for m in members], dtype=torch.int32, device="cuda")
                rows = torch.tensor([(m[2][0], m[2][1], boxes[m[0]][2], boxes[m[0]][3], flips[m[0]], m[0]) for m in members],
                                    dtype=torch.int32, device="cuda")
                res.append((buf, sizes, tab, shape, rows))
            return res

        def crops_dev(res, result):
            for buf, sizes, tab, shape, rows in res:
                rec = c.decode(wins_status(buf, sizes, tab, shape, max_pixels=max_pixels)[0])
                c.resample_boxes(rec, rows, SIZE, torch.float16, MEAN, STD, out=result)
            return result

        def base_dev(dtype=torch.float16):
            return torch.cat([torch_tail(c.decode(win_status(b, s, h8, w8, win)[0])[:, oy:oy + bh, ox:ox + bw], flip, dtype)
                              for (b, s, h8, w8, win, oy, ox, bh, bw), flip in zip(singles, flips)])

        def base_host(dtype=torch.float16):
            return torch.cat([torch_tail(dec.decode_region([f], box), flip, dtype) for f, box, flip in zip(files, boxes, flips)])

        # agreement first, in fp32
        ref = base_host(torch.float32).double()
        got = dec.decode_crops(files, boxes, SIZE, flip=flips, mean=MEAN, std=STD, dtype=torch.float32)
        assert torch.equal(dec.decode_crops(files, boxes, SIZE, flip=flips, mean=MEAN, std=STD, dtype=torch.float32, bucket=8), got)
        taps = torch.tensor([[4 + math.ceil(2 * max(b[2] / SIZE[0], 1)) + 1 + math.ceil(2 * max(b[3] / SIZE[1], 1)) + 1]
                             for b in boxes], dtype=torch.float64, device="cuda").view(FILES, 1, 1, 1)
        tol = (2 * taps * 2.0 ** -23 + 2.0 ** -22 * max(SIZE)) / std_t.double() + 2 * 2.0 ** -23 * ref.abs()
        use = float(((got.double() - ref).abs() / tol).max())
        assert use <= 1.0, use
        res_none, res_b8 = resident(None), resident(8)
        result = torch.empty((FILES, 3, *SIZE), dtype=torch.float16, device="cuda")
        half = dec.decode_crops(files, boxes, SIZE, flip=flips, mean=MEAN, std=STD, dtype=torch.float16)
        assert torch.equal(crops_dev(res_none, result), half) and torch.equal(crops_dev(res_b8, result), half)
        recs = [(c.decode(wins_status(buf, sizes, tab, shape, max_pixels=max_pixels)[0]), rows) for buf, sizes, tab, shape, rows in res_none]

        def resample_only():
            for rec, rows in recs:
                c.resample_boxes(rec, rows, SIZE, torch.float16, MEAN, STD, out=result)

        calls = {"pixels_dev_none_ms": lambda: crops_dev(res_none, result), "pixels_dev_b8_ms": lambda: crops_dev(res_b8, result),
                 "pixels_dev_baseline_ms": base_dev,
                 "pixels_none_ms": lambda: dec.decode_crops(files, boxes, SIZE, flip=flips, mean=MEAN, std=STD, dtype=torch.float16),
                 "pixels_b8_ms": lambda: dec.decode_crops(files, boxes, SIZE, flip=flips, mean=MEAN, std=STD, dtype=torch.float16,
                                                          bucket=8),
                 "pixels_baseline_ms": base_host, "resample_ms": resample_only}
        times = {k: [] for k in calls}
        for _ in range(args.rounds):  # the forms alternate, so a drift of the machine shows in all
            for k, fn in calls.items():
                times[k].append(median_ms(torch, fn, args.warmup, args.iters))
        out[f"v{ver}"] = {"groups_none": [list(r[3]) + [int(r[2].shape[0])] for r in res_none], "groups_b8": len(res_b8),
                          "groups_baseline": FILES, "agreement_use_of_allowance": round(use, 4),
                          "window_pixels_none": sum(r[3][0] * r[3][1] * int(r[2].shape[0]) for r in res_none),
                          "window_pixels_b8": sum(r[3][0] * r[3][1] * int(r[2].shape[0]) for r in res_b8), **times}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
