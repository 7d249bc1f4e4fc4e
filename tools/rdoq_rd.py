"""What rate-distortion optimised quantisation (Codec.rdoq) buys, measured: for
the trained codec of each of the three coefficients, both priors fitted on the first 200 files
(sorted) of data/imagenet_patches_1k as section 13 does, the next 200 patches and the 64 kodim21 256^2
tiles coded at every lambda of LAMS -- the static prior's choice into version-2 files, the context
prior's into version-3 files -- with the mean file bytes, the PSNR over the set, the mean MS-SSIM
(nic_sq_err / nic_ms_ssim; the 128^2 patches are below MS-SSIM's 161 pixels, so theirs is null) and
the share of codes changed.

Then the device time of Codec.rdoq (nic_rdoq) beside Codec.rans3_encode on the two batches of
section 10 (64 x 32 x 32 x 96 and 1 x 270 x 480 x 96, coefficient 0.01, lambda 0.05): hipEvents on the
current stream, the median of `--iters` calls after `--warmup`, the calls alternating, `--rounds`
medians each, all reported.

Output: profiles/rdoq_rd.json (--out) and the same JSON on one line.  Needs the GPU and the built
library."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAMS = (0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0)
COEFS = ("0.01", "0.02", "0.03")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdoq_rd.json"))
    args = ap.parse_args()
    import torch
    from PIL import Image

    from neural_network_image_compression_amd import bitstream as B
    from neural_network_image_compression_amd import weights as W
    from neural_network_image_compression_amd.codec import Codec
    from neural_network_image_compression_amd.prior import ContextPrior, Prior
    from tools.compress_bench import tiles
    from tools.png_device_times import median_ms

    d = os.path.join(ROOT, "data", "imagenet_patches_1k")
    names = B.list_dataset(d)[:400]
    patches = np.stack([np.array(Image.open(os.path.join(d, fn)).convert("RGB")) for fn in names])
    sets = {"heldout_200_patches": torch.from_numpy(patches[200:]).cuda(),
            "kodim21_64_tiles": torch.from_numpy(np.ascontiguousarray(np.stack(tiles(64)))).cuda()}
    fit = torch.from_numpy(patches[:200]).cuda()
    out = {"tool": "rdoq_rd", "lams": list(LAMS), "seg_pixels": 32, "fitted_on": "imagenet_patches_1k[0:200]",
           "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "codecs": {}}

    def quality(c, x, z):
        rec = c.decode(z)[:, :x.shape[1], :x.shape[2]].contiguous()
        ms = float(c.ms_ssim(x, rec).double().mean()) if min(x.shape[1:3]) >= 161 else None
        return c.psnr(x, rec), ms

    for coef in COEFS:
        pre = os.path.join(ROOT, "tests", "golden", "trained", f"coef{coef}_")
        c = Codec(0)
        c.set_weights({**W.load(pre + "encoder", "encoder"), **W.load(pre + "decoder", "decoder")})
        zfit = c.encode(fit)
        static = Prior.accumulator(c).add(zfit).build()
        cprior = ContextPrior.accumulator(c, static).add(zfit).build()
        c.set_prior(static)
        c.set_context_prior(cprior)
        rec = {"prior_id": f"{static.id:08x}", "context_prior_id": f"{cprior.id:08x}"}
        for name, x in sets.items():
            z, f = c.encode(x, prequant=True)
            rows = []
            for lam in LAMS:
                row = {"lam": lam}
                for ver, kind, enc in ((2, "static", c.rans2_encode), (3, "context", c.rans3_encode)):
                    zq = c.rdoq(z, f, lam, prior=kind)
                    if lam == 0.0:
                        assert bool((zq == z).all()), "lambda 0 is not the identity"
                    buf, sizes = enc(zq)
                    assert bool(((c.rans2_decode if ver == 2 else c.rans3_decode)(buf, sizes, *z.shape[1:3]) == zq).all())
                    psnr, ms = quality(c, x, zq)
                    row[f"v{ver}"] = {"mean_file_bytes": float(sizes.double().mean()), "psnr_db": psnr, "ms_ssim": ms,
                                      "codes_changed": float((zq != z).double().mean())}
                rows.append(row)
                print(f"coef {coef} {name} {json.dumps(row)}", file=sys.stderr, flush=True)
            rec[name] = rows
        out["codecs"][coef] = rec
        if coef == COEFS[0]:  # device times, on section 10's two batches
            with np.load(os.path.join(ROOT, "tests", "golden", "kodim21_full.npz"), allow_pickle=False) as g:
                full = g["x"][0]
            frame = np.tile(full, (2160 // full.shape[0] + 1, 3840 // full.shape[1] + 1, 1))[:2160, :3840]
            times = {}
            for name, x in (("64x32x32x96", sets["kodim21_64_tiles"]), ("1x270x480x96", torch.from_numpy(np.ascontiguousarray(frame[None])).cuda())):
                z, f = c.encode(x, prequant=True)
                n, h8, w8, _ = z.shape
                c.rans3_reserve(n, h8, w8)
                buf = torch.empty_like(z)
                calls = {"rdoq_context_ms": lambda: c.rdoq(z, f, 0.05, prior="context", out=buf),
                         "rdoq_static_ms": lambda: c.rdoq(z, f, 0.05, prior="static", out=buf),
                         "rans3_encode_ms": lambda: c.rans3_encode(z)}
                t = {k: [] for k in calls}
                for _ in range(args.rounds):  # the calls alternate, so a drift of the box shows in all
                    for k, fn in calls.items():
                        t[k].append(median_ms(torch, fn, args.warmup, args.iters))
                times[name] = {"latent": list(z.shape), "lam": 0.05, **t}
            out["device_times"] = times
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
