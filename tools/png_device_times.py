"""Device time of the device PNG writer (Codec.png_encode) beside the decoder pass that makes its
input, on the two batches of DESIGN.md: 64 reconstructions of 256^2 kodim21 tiles (trained coef-0.01
codec) and one 2160x3840 frame.  hipEvents on the current stream, the median of `--iters` calls
after `--warmup`; workspaces are reserved first, so no call allocates.

Output: one JSON line.  Needs the GPU and the built library."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(torch, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch

    from neural_network_image_compression_amd import weights as W
    from neural_network_image_compression_amd.codec import Codec
    from tools.compress_bench import tiles

    pre = os.path.join(ROOT, "tests", "golden", "trained", "coef0.01_")
    w = W.load(pre + "encoder", "encoder")
    w.update(W.load(pre + "decoder", "decoder"))
    c = Codec(0)
    c.set_weights(w)
    with np.load(os.path.join(ROOT, "tests", "golden", "kodim21_full.npz"), allow_pickle=False) as g:
        full = g["x"][0]
    frame = np.tile(full, (2160 // full.shape[0] + 1, 3840 // full.shape[1] + 1, 1))[:2160, :3840]
    out = {"tool": "png_device_times", "iters": args.iters, "block_bytes": int(c._L.nic_png_device_block_bytes())}
    for name, x in (("64x256x256", np.stack(tiles(64))), ("1x2160x3840", frame[None])):
        z = c.encode(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        rec = c.decode(z)
        n, h, wd, _ = rec.shape
        c.reserve(n, h, wd)
        c.png_reserve(n, h, wd, 3)
        buf, sizes = c.png_encode(rec)
        dec_ms = median_ms(torch, lambda: c.decode(z, out=rec), args.warmup, args.iters)
        png_ms = median_ms(torch, lambda: c.png_encode(rec), args.warmup, args.iters)
        out[name] = {"images": list(rec.shape), "raw_bytes_per_image": int(h * wd * 3),
                     "mean_file_bytes": float(sizes.double().mean().item()), "codec_decode_ms": dec_ms,
                     "png_encode_ms": png_ms}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
