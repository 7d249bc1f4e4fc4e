"""Device time of region decode beside the full decode, in one process, on the 2160x3840 frame tiled
from kodim21 (a 270x480 latent; DESIGN.md section 10's frame) with the trained coef-0.01 codec, for
.nic versions 2 and 3 (priors fitted on the first 200 files, sorted, of data/imagenet_patches_1k, as
tools/rans3_device_times.py), seg_pixels 32, for a centred 512x512 box and a centred 64x64 box:

  entropy      Codec.rans*_decode_window_status of the box's latent window against
               Codec.rans*_decode_status of the whole latent, files resident on the device
  pixels       bitstream.decode_region (host checks, upload of the whole file, window entropy decode,
               the decoder on the window, the cut) against the same route for the whole frame:
               bitstream.read_nic, Codec.decode and the crop of the box on the device
  pixels_dev   the device part of both alone, files resident on the device: window entropy decode +
               decode + cut against full entropy decode + decode + crop

hipEvents on the current stream, the median of `--iters` calls after `--warmup`, `--rounds` such
medians per form with the two forms alternating (all reported); workspaces are reserved first.
Every region result is first checked equal to the crop of the full decode.

Output: one JSON line.  Needs the GPU and the built library."""
import argparse
import ctypes
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

    from neural_network_image_compression_amd import _lib
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
    H, Wd = 2160, 3840
    frame = np.tile(full, (H // full.shape[0] + 1, Wd // full.shape[1] + 1, 1))[:H, :Wd]
    lat = c.encode(torch.from_numpy(np.ascontiguousarray(frame[None])).cuda())
    n, h8, w8, _ = lat.shape
    out = {"tool": "region_decode_times", "iters": args.iters, "rounds": args.rounds, "prior_id": f"{static.id:08x}",
           "context_prior_id": f"{cprior.id:08x}", "fitted_on": "imagenet_patches_1k[0:200]", "frame": [H, Wd],
           "latent": list(lat.shape), "seg_pixels": B.NIC_SEG_PIXELS}
    c.reserve(1, H, Wd)

    def window_segments(win):
        count = ctypes.c_int64()
        _lib.check(_lib.lib().nic_rans_window_segments(h8, w8, B.NIC_SEG_PIXELS, *win, ctypes.byref(count)),
                   "nic_rans_window_segments")
        return count.value

    for ver in (2, 3):
        c.set_prior(static if ver == 2 else None)  # nic_files writes version 3 when a context prior is set
        c.set_context_prior(cprior if ver == 3 else None)
        (c.rans2_reserve if ver == 2 else c.rans3_reserve)(n, h8, w8)
        buf, sizes = (c.rans2_encode if ver == 2 else c.rans3_encode)(lat)
        data = B.nic_files(c, lat)[0]
        assert data[4] == ver
        full_status = c.rans2_decode_status if ver == 2 else c.rans3_decode_status
        win_status = c.rans2_decode_window_status if ver == 2 else c.rans3_decode_window_status
        assert bool((full_status(buf, sizes, h8, w8)[0] == lat).all())
        whole = c.decode(lat)
        res = {"file_bytes": len(data), "segments": -(-h8 * w8 // B.NIC_SEG_PIXELS)}
        for side in (512, 64):
            box = ((H - side) // 2, (Wd - side) // 2, side, side)
            y0, x0 = box[:2]
            win, (oy, ox) = Codec.region_plan(H, Wd, box)
            assert bool((dec.decode_region([data], box) == whole[:, y0:y0 + side, x0:x0 + side]).all())

            def region_dev():
                zw = win_status(buf, sizes, h8, w8, win)[0]
                return c.decode(zw)[:, oy:oy + side, ox:ox + side].contiguous()

            def full_dev():
                zf = full_status(buf, sizes, h8, w8)[0]
                return c.decode(zf)[:, y0:y0 + side, x0:x0 + side].contiguous()

            def full_host():
                (zf,) = B.read_nic(c, [data])
                return c.decode(zf[None])[:, y0:y0 + side, x0:x0 + side].contiguous()

            assert bool((region_dev() == full_dev()).all())
            calls = {"entropy_window_ms": lambda: win_status(buf, sizes, h8, w8, win),
                     "entropy_full_ms": lambda: full_status(buf, sizes, h8, w8),
                     "pixels_region_ms": lambda: dec.decode_region([data], box), "pixels_full_ms": full_host,
                     "pixels_dev_region_ms": region_dev, "pixels_dev_full_ms": full_dev}
            times = {k: [] for k in calls}
            for _ in range(args.rounds):  # the forms alternate, so a drift of the box shows in both
                for k, fn in calls.items():
                    times[k].append(median_ms(torch, fn, args.warmup, args.iters))
            res[f"box{side}"] = {"box": list(box), "window": list(win),
                                 "window_segments": window_segments(win), **times}
        out[f"v{ver}"] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
