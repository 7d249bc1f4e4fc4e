#!/usr/bin/env python
"""Fit the .nic version-3 context prior of a checkpoint over a directory of images and write a .nicc.

    python tools/fit_context_prior.py DATASET CHECKPOINT OUT.nicc [--batch-size 64] [--seg-pixels 32]

CHECKPOINT is the encoder's prefix (as Encoder.compress takes it).  Two passes over the colour
images of DATASET (sorted; read_dataset's filter), each decoding them with the driver's reader pool
and encoding consecutive equal-shaped images as one device batch: the first counts the latents into
the static prior (Prior.accumulator), whose rows' argmax are the anchors; the second counts them per
context (ContextPrior.accumulator) for segments of --seg-pixels latent pixels, the segment size of
the files the drivers write.  Both normalisations run on the device; the context prior goes to OUT.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("dataset")
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--seg-pixels", type=int, default=None, help="default: the drivers' segment size")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch

    from neural_network_image_compression_amd import bitstream as B
    from neural_network_image_compression_amd.codec import Encoder
    from neural_network_image_compression_amd.prior import ContextPrior, Prior

    seg_pixels = B.NIC_SEG_PIXELS if args.seg_pixels is None else args.seg_pixels
    enc = Encoder(args.device)
    enc.load(args.checkpoint)
    files = B.list_dataset(args.dataset)

    def sweep(acc):
        """Every image's latent into acc; -> the number of images."""
        batch, images = [], 0

        def flush():
            if batch:
                acc.add(enc.codec.encode(torch.from_numpy(np.stack(batch)).to(f"cuda:{args.device}")))
                batch.clear()

        with ThreadPoolExecutor(max_workers=min(8, B._host_threads())) as readers:
            for a in readers.map(B._read_one, [os.path.join(args.dataset, fn) for fn in files]):
                if a.ndim != 3:  # read_dataset keeps colour (3-D) images only
                    continue
                if batch and (a.shape != batch[0].shape or len(batch) >= args.batch_size
                              or (len(batch) + 1) * a.shape[0] * a.shape[1] > B.BATCH_PIXELS):
                    flush()
                batch.append(a.astype(np.uint8, copy=False))
                images += 1
            flush()
        return images

    static = Prior.accumulator(enc.codec)
    sweep(static)
    acc = ContextPrior.accumulator(enc.codec, static.build(), seg_pixels)
    images = sweep(acc)
    cprior = acc.build()
    cprior.save(args.out)
    print(f"{args.out}: context prior {cprior.id:08x} over {images} images, {int(acc.counts[0].sum())} latent pixels, "
          f"segments of {seg_pixels}")


if __name__ == "__main__":
    main()
