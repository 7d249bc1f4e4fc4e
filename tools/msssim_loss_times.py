"""Device time of the MS-SSIM training loss on HIP beside what the library could do before it, in
one process, at the training shape: 64 planes of 128 x 128, K = 4 scales.

  loss         forward plus backward (gradient to the decoded plane) of the loss alone:
               train_hip.ms_ssim_mean against the baseline, the fp32 PyTorch restatement
               training.ms_ssim(hip=False) -- backend="torch"'s loss -- on the same tensors; and
               loss_ssim_hip, the single-scale training.ssim(hip=True) alone on those tensors (the
               default loss, which train_step_ssim's total hides)
  train_step   Training.train_step on a batch of 64 patches (192 planes through the codec, the
               loss on 64 Y and 128 CbCr planes), backend "hip", with distortion "ms_ssim"
               (HIP loss), with distortion "ms_ssim" and the loss on the PyTorch restatement, and
               with distortion "ssim" (the default), so the cost of the richer loss shows

hipEvents on the current stream, the median of `--iters` calls after `--warmup`, `--rounds` such
medians per form with the forms alternating (all reported).  Before timing, the HIP loss and its
gradient are checked against the restatement (1e-4 of the largest reference value).

Output: one JSON line, also written to --out.  Needs the GPU and the built library."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, iters, warmup):
    import torch

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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--scales", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_loss_times.json"))
    args = ap.parse_args()
    import torch

    from neural_network_image_compression_amd import train_hip
    from neural_network_image_compression_amd import training as T
    from neural_network_image_compression_amd import weights as W

    if not torch.cuda.is_available():
        raise SystemExit("msssim_loss_times: needs the GPU")
    n, s, k = args.planes, args.size, args.scales
    g = torch.Generator().manual_seed(0)
    yy = torch.linspace(0, 1, s).view(1, 1, s, 1)
    xx = torch.linspace(0, 1, s).view(1, 1, 1, s)
    x = (0.5 + 0.3 * torch.sin(6.28 * yy) * torch.cos(9.42 * xx) + 0.15 * (torch.rand((n, 1, s, s), generator=g) - 0.5))
    x = x.clamp(0, 1).cuda()
    y0 = (x + 0.05 * torch.randn(x.shape, generator=g).cuda()).clamp(0, 1)

    def loss_fn(hip):
        def run():
            y = y0.detach().requires_grad_()
            v = train_hip.ms_ssim_mean(x, y, k) if hip else T.ms_ssim(x, y, scales=k, hip=False)
            (gy,) = torch.autograd.grad(((1 - v.mean()) / 2), y)
            return v, gy
        return run

    def loss_ssim_hip():
        y = y0.detach().requires_grad_()
        v = T.ssim(x, y, hip=True)
        return v, torch.autograd.grad(((1 - v.mean()) / 2), y)[0]

    v_h, g_h = loss_fn(True)()
    v_t, g_t = loss_fn(False)()
    dv = float((v_h - v_t).detach().abs().max() / v_t.detach().abs().max())
    dg = float((g_h - g_t).abs().max() / g_t.abs().max())
    if not (dv <= 1e-4 and dg <= 1e-4):
        raise SystemExit(f"msssim_loss_times: HIP loss differs from the restatement: value {dv:.2e} gradient {dg:.2e}")

    rng = np.random.default_rng(0)
    a = np.cumsum(np.cumsum(rng.integers(-2, 3, (n, s, s, 3)), axis=1), axis=2).astype(np.float64)
    a -= a.min(axis=(1, 2, 3), keepdims=True)
    imgs = torch.from_numpy((a * 255.0 / np.maximum(a.max(axis=(1, 2, 3), keepdims=True), 1)).astype(np.uint8))

    def step_fn(distortion, hip_loss):
        tr = T.Training(device="cuda", weights=W.seeded_weights(0, init="glorot"), seed=0, distortion=distortion,
                        ms_scales=k)
        real = T.ms_ssim

        def run():
            if not hip_loss:  # the codec on HIP, the loss on the PyTorch restatement
                T.ms_ssim = lambda p, q, scales=4, max_val=1.0, hip=False: real(p, q, scales, max_val, False)
            try:
                tr.train_step(imgs, 0.01)
            finally:
                T.ms_ssim = real
        return run

    forms = {"loss_hip": loss_fn(True), "loss_ssim_hip": loss_ssim_hip, "loss_torch_fp32": loss_fn(False),
             "train_step_ms_ssim_hip_loss": step_fn("ms_ssim", True),
             "train_step_ms_ssim_torch_loss": step_fn("ms_ssim", False),
             "train_step_ssim": step_fn("ssim", True)}
    res = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            res[name].append(round(median_ms(fn, args.iters, args.warmup), 4))
    out = {"tool": "msssim_loss_times", "device": torch.cuda.get_device_name(0), "planes": n, "size": s, "scales": k,
           "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds,
           "check": {"value_rel": dv, "gradient_rel": dg},
           "median_ms": res,
           "note": "train_step: 64 patches, host PNG target and optimiser included; loss: forward + backward alone"}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
