"""Device time of the device PNG reader (Codec.png_read_status) beside the encoder pass that takes its
output, on the batches of DESIGN.md: 64 256^2 kodim21 tiles in Pillow's optimize=True files and in the
device writer's files, and one 2160x3840 frame in Pillow's file; for the frame also Pillow's own
decode time on one host thread.  hipEvents on the current stream, the median of `--iters` calls after
`--warmup`, `--medians` such medians; workspaces are reserved first, so no call allocates.

Output: one JSON line.  Needs the GPU and the built library."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.png_device_times import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--medians", type=int, default=3)
    args = ap.parse_args()
    import torch
    from PIL import Image

    from neural_network_image_compression_amd import bitstream as B
    from neural_network_image_compression_amd import weights as W
    from neural_network_image_compression_amd.codec import Codec
    from tools.compress_bench import tiles

    c = Codec(0)
    c.set_weights(W.load(os.path.join(ROOT, "tests", "golden", "trained", "coef0.01_") + "encoder", "encoder"))
    with np.load(os.path.join(ROOT, "tests", "golden", "kodim21_full.npz"), allow_pickle=False) as g:
        full = g["x"][0]
    frame = np.ascontiguousarray(np.tile(full, (2160 // full.shape[0] + 1, 3840 // full.shape[1] + 1, 1))[:2160, :3840])
    x64 = np.stack(tiles(64))
    sets = (("64x256x256 pillow files", x64, [B.png_bytes(a) for a in x64]),
            ("64x256x256 device-writer files", x64, B.png_files_device(c, torch.from_numpy(x64).cuda())),
            ("1x2160x3840 pillow file", frame[None], [B.png_bytes(frame)]))
    out = {"tool": "png_read_times", "iters": args.iters, "medians": args.medians}
    for name, x, files in sets:
        n, h, w, _ = x.shape
        streams = [B.png_stream(f)[3] for f in files]
        buf, lens = B._upload_files(c, streams)
        dev = torch.from_numpy(x).cuda()
        c.reserve(n, h, w)
        c.png_read_reserve(n, h, w, 3)
        images, status = c.png_read_status(buf, lens, h, w, 3)
        assert status.cpu().tolist() == [0] * n and torch.equal(images, dev)
        z = c.encode(dev)
        t0 = time.perf_counter()
        for f in files:
            with Image.open(io.BytesIO(f)) as im:
                np.array(im)
        host_ms = (time.perf_counter() - t0) * 1e3
        out[name] = {"images": [n, h, w, 3], "mean_stream_bytes": float(np.mean([len(s) for s in streams])),
                     "png_read_ms": [median_ms(torch, lambda: c.png_read_status(buf, lens, h, w, 3, out=images), args.warmup, args.iters)
                                     for _ in range(args.medians)],
                     "codec_encode_ms": [median_ms(torch, lambda: c.encode(dev, out=z), args.warmup, args.iters)
                                         for _ in range(args.medians)],
                     "pillow_one_thread_ms": round(host_ms, 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
