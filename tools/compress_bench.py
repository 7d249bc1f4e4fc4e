"""Directory throughput of the reference's file-level API: Encoder.compress /
Decoder.uncompress (encoder.py:49-51, decoder.py:50-52, utils.py:30-62, 85-87) on a directory of
256^2 RGB PNG tiles cut from kodim21 (the reference's validation image; 6 tiles, flipped and
shifted into `--images` distinct ones).  Reports images/s and MP/s per driver mode (the reference's serial loop, round 4's threaded
writes, round 5's pipeline) on the kodim21 tiles and on data/imagenet_patches_1k, and whether
every mode wrote the same bytes.

`--container png nic` (the default measures both after the driver modes; naming containers runs
only this part) compares the on-disk containers in one run on the kodim21 tiles with the default
pipeline: the reference's packed PNG against the device-coded .nic (bitstream.py), images/s of
compress / uncompress, the mean file size of each, and whether both routes reconstruct the same
PNGs.  `--weights trained` (default for this part) uses the committed coef-0.01 codec, whose
latents are what the containers are meant for; `spread` the seeded dense ones.
`--png-writer pillow device` loops the reconstruction writers of uncompress as well (Pillow's
encoder on host threads against the device PNG writer): every (container, writer) pair in the same
run, keyed "<container>+<writer>", with every repeat's uncompress time, the mean size of the
reconstruction files and whether all pairs decode to the same pixels.

Output: one JSON line.  Needs the GPU (the codec) and the built library."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tiles(n):
    with np.load(os.path.join(ROOT, "tests", "golden", "kodim21_full.npz"), allow_pickle=False) as g:
        x = g["x"][0]
    base = [x[y:y + 256, xx:xx + 256] for y in (0, 256) for xx in (0, 256, 512)] if x.shape[0] >= 512 else []
    if not base:
        base = [x[y:y + 256, xx:xx + 256] for y in (0, 256, 512) for xx in (0, 256)]
    out = []
    k = 0
    while len(out) < n:
        t = base[k % len(base)]
        v = k // len(base)
        t = np.roll(t, (3 * v) % 256, axis=1)
        if v & 1:
            t = t[:, ::-1]
        if v & 2:
            t = t[::-1]
        out.append(np.ascontiguousarray(t))
        k += 1
    return out


def run_modes(enc, dec, tmp, ds, ck, n, px, modes, repeat):
    """Best-of-`repeat` compress / uncompress wall time per driver mode (after a warm-up round)."""
    res, files = {}, {}
    for name, kw in modes:
        best = {}
        for r in range(repeat + 1):  # the first round warms up (HIP modules, page cache)
            for d in (os.path.basename(ds) + "_compressed", os.path.basename(ds) + "_uncompressed"):
                shutil.rmtree(os.path.join(tmp, d), ignore_errors=True)
            t0 = time.perf_counter()
            enc.compress(ds, os.path.join(ck, "encoder"), **kw)
            t1 = time.perf_counter()
            dec.uncompress(ds + "_compressed", os.path.join(ck, "decoder"), **kw)
            t2 = time.perf_counter()
            if r:
                best["compress_s"] = min(best.get("compress_s", 1e9), t1 - t0)
                best["uncompress_s"] = min(best.get("uncompress_s", 1e9), t2 - t1)
        out = {k: round(v, 4) for k, v in best.items()}
        out.update({"compress_img_s": round(n / best["compress_s"], 1), "uncompress_img_s": round(n / best["uncompress_s"], 1),
                    "compress_MP_s": round(n * px / 1e6 / best["compress_s"], 2),
                    "uncompress_MP_s": round(n * px / 1e6 / best["uncompress_s"], 2), "args": kw})
        res[name] = out
        files[name] = {d: {f: open(os.path.join(ds + d, f), "rb").read() for f in sorted(os.listdir(ds + d))}
                       for d in ("_compressed", "_uncompressed")}
    same = all(files[k] == files[modes[0][0]] for k in files)
    return res, same


def recon_pixels(path):
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im).tobytes()


def run_containers(enc, dec, tmp, ds, ck, n, px, containers, repeat, writers=None, readers=None):
    """Best-of-`repeat` compress / uncompress wall time and mean file size per container (and per
    reconstruction writer and PNG reader, when they are named; both repeats of every figure are
    listed then)."""
    res, recon = {}, {}
    for cont, writer, reader in [(c, w, r) for c in containers for w in (writers or [None]) for r in (readers or [None])]:
        best, runs, cruns = {}, [], []
        ukw = {"png_writer": writer} if writer else {}
        ckw = {"png_reader": reader} if reader else {}
        if reader and cont == "png":
            ukw["png_reader"] = reader  # the decoder side of "nic" reads no PNG
        for r in range(repeat + 1):
            for d in ("_compressed", "_uncompressed"):
                shutil.rmtree(ds + d, ignore_errors=True)
            t0 = time.perf_counter()
            enc.compress(ds, os.path.join(ck, "encoder"), container=cont, **ckw)
            t1 = time.perf_counter()
            dec.uncompress(ds + "_compressed", os.path.join(ck, "decoder"), container=cont, **ukw)
            t2 = time.perf_counter()
            if r:
                best["compress_s"] = min(best.get("compress_s", 1e9), t1 - t0)
                best["uncompress_s"] = min(best.get("uncompress_s", 1e9), t2 - t1)
                runs.append(round(t2 - t1, 4))
                cruns.append(round(t1 - t0, 4))
        sizes = [os.path.getsize(os.path.join(ds + "_compressed", f)) for f in os.listdir(ds + "_compressed")]
        key = f"{cont}+{writer}" if writer else cont
        if reader:
            key += f"+read:{reader}"
        if writer:
            rs = [os.path.getsize(os.path.join(ds + "_uncompressed", f)) for f in os.listdir(ds + "_uncompressed")]
            res[key] = {"uncompress_s_runs": runs, "mean_recon_file_bytes": round(float(np.mean(rs)), 1)}
            recon[key] = {f: recon_pixels(os.path.join(ds + "_uncompressed", f)) for f in sorted(os.listdir(ds + "_uncompressed"))}
        else:
            res[key] = {}
            recon[key] = {f: open(os.path.join(ds + "_uncompressed", f), "rb").read()
                          for f in sorted(os.listdir(ds + "_uncompressed"))}
        res[key].update({"compress_s": round(best["compress_s"], 4), "uncompress_s": round(best["uncompress_s"], 4),
                     "compress_img_s": round(n / best["compress_s"], 1),
                     "uncompress_img_s": round(n / best["uncompress_s"], 1),
                     "compress_MP_s": round(n * px / 1e6 / best["compress_s"], 2),
                     "uncompress_MP_s": round(n * px / 1e6 / best["uncompress_s"], 2),
                     "files": len(sizes), "mean_file_bytes": round(float(np.mean(sizes)), 1)})
        if reader:
            res[key]["compress_s_runs"] = cruns
    same = all(recon[c] == next(iter(recon.values())) for c in recon)
    return res, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--container", nargs="+", choices=("png", "nic"), default=None,
                    help="compare these on-disk containers only (default: the driver modes, then both)")
    ap.add_argument("--png-writer", nargs="+", choices=("pillow", "device"), default=None,
                    help="also loop these reconstruction writers of uncompress (default: Pillow's only)")
    ap.add_argument("--png-reader", nargs="+", choices=("pillow", "device"), default=None,
                    help="also loop these PNG readers of compress and of uncompress from the PNG container")
    ap.add_argument("--weights", choices=("trained", "spread"), default="trained",
                    help="codec of the container comparison")
    ap.add_argument("--images", type=int, default=192)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--imagenet", default=os.path.join(ROOT, "data", "imagenet_patches_1k"))
    args = ap.parse_args()
    from PIL import Image

    from neural_network_image_compression_amd import weights as W
    from neural_network_image_compression_amd.codec import Decoder, Encoder

    tmp = tempfile.mkdtemp(prefix="nic_compress_")
    try:
        ds = os.path.join(tmp, "tiles")
        os.makedirs(ds)
        for i, t in enumerate(tiles(args.images)):
            Image.fromarray(t).save(os.path.join(ds, f"t{i:05d}.png"))
        ck = os.path.join(tmp, "ck")
        w = W.seeded_weights(0, init="spread")
        W.save(w, os.path.join(ck, "encoder"), "encoder")
        W.save(w, os.path.join(ck, "decoder"), "decoder")
        enc, dec = Encoder(0), Decoder(0)
        # the reference's serial loop (utils.py:46-62: batches of 4, each saved inline), round 4's
        # default (batches of 4, PNG writes on 8 threads behind the device), round 5's pipeline
        modes = [("serial_b4", {"batch_size": 4, "workers": 0}), ("r4_b4_w8", {"batch_size": 4, "workers": 8}),
                 ("pipeline_b64", {})]
        out = {"tool": "compress_bench", "host_cpus": len(os.sched_getaffinity(0))}
        if args.container is None and args.png_writer is None and args.png_reader is None:
            res, same = run_modes(enc, dec, tmp, ds, ck, args.images, 65536, modes, args.repeat)
            out["kodim21_tiles"] = {"images": args.images, "tile": "256x256x3 kodim21 tiles", "modes": res,
                                    "files_identical_across_modes": same}
        ckc = ck
        if args.weights == "trained":
            ckc = os.path.join(tmp, "ck_trained")
            pre = os.path.join(ROOT, "tests", "golden", "trained", "coef0.01_")
            W.save(W.load(pre + "encoder", "encoder"), os.path.join(ckc, "encoder"), "encoder")
            W.save(W.load(pre + "decoder", "decoder"), os.path.join(ckc, "decoder"), "decoder")
        res, same = run_containers(enc, dec, tmp, ds, ckc, args.images, 65536, args.container or ["png", "nic"],
                                   args.repeat, writers=args.png_writer, readers=args.png_reader)
        out["containers"] = {"images": args.images, "tile": "256x256x3 kodim21 tiles", "weights": args.weights,
                             "driver": "pipeline_b64", "by_container": res, "reconstructions_identical": same}
        if args.png_writer:  # files differ between writers by design: the comparison is of decoded pixels
            out["containers"]["compared"] = "decoded pixels"
        if args.container is None and args.png_writer is None and args.png_reader is None and os.path.isdir(args.imagenet):
            inet = os.path.join(tmp, "inet")
            shutil.copytree(args.imagenet, inet)
            n = len([f for f in os.listdir(inet) if f.endswith(".jpg")])
            res, same = run_modes(enc, dec, tmp, inet, ck, n, 128 * 128, modes, args.repeat)
            out["imagenet_patches_1k"] = {"images": n, "tile": "128x128x3 JPEG patches", "modes": res,
                                          "files_identical_across_modes": same}
        print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
