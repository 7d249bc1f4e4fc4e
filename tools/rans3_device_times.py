"""Device time and file sizes of the .nic container's version 3 beside versions 1 and 2, in one
process: Codec.rans_encode / rans_decode, rans2_encode / rans2_decode and rans3_encode / rans3_decode on the two batches of
DESIGN.md section 10 (64 latents of 256^2 kodim21 tiles and one 270x480 latent of a 2160x3840
frame, trained coef-0.01 codec), hipEvents on the current stream, the median of `--iters` calls after
`--warmup`, the two versions alternating (`--rounds` medians each, all reported); workspaces are
reserved first.  Both priors are fitted on the first 200 files (sorted) of data/imagenet_patches_1k;
the mean file sizes of the three versions are taken on the next 200 and on the 64 tiles.

Output: one JSON line.  Needs the GPU and the built library."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    from neural_network_image_compression_amd.codec import Codec
    from neural_network_image_compression_amd.prior import ContextPrior, Prior
    from tools.compress_bench import tiles
    from tools.png_device_times import median_ms

    pre = os.path.join(ROOT, "tests", "golden", "trained", "coef0.01_")
    c = Codec(0)
    c.set_weights(W.load(pre + "encoder", "encoder"))
    d = os.path.join(ROOT, "data", "imagenet_patches_1k")
    names = B.list_dataset(d)[:400]
    x = np.stack([np.array(Image.open(os.path.join(d, fn)).convert("RGB")) for fn in names])
    z = torch.cat([c.encode(torch.from_numpy(x[i:i + 100]).cuda()) for i in range(0, 400, 100)])
    static = Prior.accumulator(c).add(z[:200]).build()
    cprior = ContextPrior.accumulator(c, static).add(z[:200]).build()
    c.set_prior(static)
    c.set_context_prior(cprior)
    with np.load(os.path.join(ROOT, "tests", "golden", "kodim21_full.npz"), allow_pickle=False) as g:
        full = g["x"][0]
    frame = np.tile(full, (2160 // full.shape[0] + 1, 3840 // full.shape[1] + 1, 1))[:2160, :3840]
    out = {"tool": "rans3_device_times", "iters": args.iters, "rounds": args.rounds, "prior_id": f"{static.id:08x}",
           "context_prior_id": f"{cprior.id:08x}", "fitted_on": "imagenet_patches_1k[0:200]"}

    def mean_sizes(lat):
        return {"v1": float(c.rans_encode(lat)[1].double().mean()), "v2": float(c.rans2_encode(lat)[1].double().mean()),
                "v3": float(c.rans3_encode(lat)[1].double().mean())}

    out["mean_file_bytes_heldout_200_patches"] = mean_sizes(z[200:])
    for name, img in (("64x256x256", np.stack(tiles(64))), ("1x2160x3840", frame[None])):
        lat = c.encode(torch.from_numpy(np.ascontiguousarray(img)).cuda())
        n, h8, w8, _ = lat.shape
        c.rans_reserve(n, h8, w8)
        c.rans2_reserve(n, h8, w8)
        c.rans3_reserve(n, h8, w8)
        b1, s1 = c.rans_encode(lat)
        b2, s2 = c.rans2_encode(lat)
        b3, s3 = c.rans3_encode(lat)
        assert bool((c.rans_decode(b1, s1, h8, w8) == lat).all())
        assert bool((c.rans2_decode(b2, s2, h8, w8) == lat).all()) and bool((c.rans3_decode(b3, s3, h8, w8) == lat).all())
        calls = {"rans_encode_ms": lambda: c.rans_encode(lat), "rans2_encode_ms": lambda: c.rans2_encode(lat),
                 "rans3_encode_ms": lambda: c.rans3_encode(lat),
                 "rans_decode_ms": lambda: c.rans_decode_status(b1, s1, h8, w8),
                 "rans2_decode_ms": lambda: c.rans2_decode_status(b2, s2, h8, w8),
                 "rans3_decode_ms": lambda: c.rans3_decode_status(b3, s3, h8, w8)}
        times = {k: [] for k in calls}
        for _ in range(args.rounds):  # the versions alternate, so a drift of the box shows in both
            for k, fn in calls.items():
                times[k].append(median_ms(torch, fn, args.warmup, args.iters))
        out[name] = {"latent": list(lat.shape), "mean_file_bytes": mean_sizes(lat), **times}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
