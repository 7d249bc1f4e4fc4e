#!/usr/bin/env python
"""Fit the .nic version-2 prior of a checkpoint over a directory of images and write a .nicp.

    python tools/fit_prior.py DATASET CHECKPOINT OUT.nicp [--batch-size 64]

CHECKPOINT is the encoder's prefix (as Encoder.compress takes it).  Every colour image of DATASET
(sorted; read_dataset's filter) is decoded by the driver's reader pool, consecutive equal-shaped
images are encoded as one device batch, and their latents are counted on the device
(Prior.accumulator); the counts are normalised there and the prior is written to OUT.
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
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch

    from neural_network_image_compression_amd import bitstream as B
    from neural_network_image_compression_amd.codec import Encoder
    from neural_network_image_compression_amd.prior import Prior

    enc = Encoder(args.device)
    enc.load(args.checkpoint)
    acc = Prior.accumulator(enc.codec)
    files = B.list_dataset(args.dataset)
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
    prior = acc.build()
    prior.save(args.out)
    print(f"{args.out}: prior {prior.id:08x} over {images} images, {int(acc.counts[0].sum())} latent pixels")


if __name__ == "__main__":
    main()
