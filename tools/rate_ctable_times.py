"""Device time of the context rate loss on HIP beside its PyTorch restatement, and what the context
rate adds to the training step, in one process, at the training shape: 192 planes of 16 x 16 x 32
(a batch of 64 patches of 128 x 128), 3 groups, segments of 32 pixels.

  forward      nic_rate_ctable alone (train_hip.rate_ctable_bits) against training.context_bits on
               the same device tensors (NCHW, as backend="torch" holds them)
  backward     nic_rate_ctable_grad with both gradients, dy alone and dL alone, against the
               restatement's autograd backward (both gradients; its forward is not in the figure)
  train_step   Training.train_step on 64 patches, backend "hip", with rate "table" (the baseline,
               unchanged) and with rate "context", alternating; wall-clock per step with a device
               synchronisation at its end, beside the hipEvent figure

hipEvents on the current stream, the median of `--iters` calls after `--warmup`, `--rounds` such
medians per form with the forms alternating (all reported).  Before timing, the HIP loss and both
gradients are checked against the restatement (1e-4 of the largest reference value).

Output: one JSON line, also written to --out.  Needs the GPU and the built library."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rate_table_times import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--seg-pixels", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_ctable_times.json"))
    args = ap.parse_args()
    import torch

    from neural_network_image_compression_amd import train_hip
    from neural_network_image_compression_amd import training as T
    from neural_network_image_compression_amd import weights as W

    if not torch.cuda.is_available():
        raise SystemExit("rate_ctable_times: needs the GPU")
    groups, c, seg = T.TABLE_GROUPS, T.TABLE_CHANNELS, args.seg_pixels
    m, hw = groups * args.batch, args.size // 8
    gen = torch.Generator().manual_seed(0)
    # a latent like the step's: a third of it clamped at 0, the rest spread; the contexts come from
    # the clean latent, the rate is taken at the noisy one
    clean = (torch.rand((m, hw, hw, c), generator=gen) * 1.5 - 0.5).clamp(0, 1)
    y = (clean + (torch.rand(clean.shape, generator=gen) - 0.5) / 255).clamp(0, 1).cuda()
    yc = clean.cuda()
    y_nchw, yc_nchw = y.permute(0, 3, 1, 2).contiguous(), yc.permute(0, 3, 1, 2).contiguous()
    L = T.context_code_lengths(torch.randn((groups * c, 3, 256), generator=gen).cuda()).contiguous()
    anchors = torch.randint(0, 4, (groups * c,), generator=gen, dtype=torch.uint8).cuda()
    g = torch.full((m,), 1.0 / (m * args.size * args.size), device="cuda")

    def torch_backward():
        yy, LL = y_nchw.detach().requires_grad_(), L.detach().requires_grad_()
        bits = T.context_bits(yy, LL, anchors, groups, seg, yc_nchw)
        return bits, lambda: torch.autograd.grad((bits * g).sum(), (yy, LL), retain_graph=True)

    bits_t, back_t = torch_backward()
    dy_t, dl_t = back_t()
    bits_h = train_hip.rate_ctable_bits(y, L, anchors, groups, seg, yc)
    dy_h, dl_h = train_hip.rate_ctable_grad(y, L, anchors, g, groups, seg, yc)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    check = {"bits_rel": rel(bits_h, bits_t.detach()), "dy_rel": rel(dy_h, dy_t.permute(0, 2, 3, 1)),
             "dL_rel": rel(dl_h, dl_t)}
    if max(check.values()) > 1e-4:
        raise SystemExit(f"rate_ctable_times: the HIP loss differs from the restatement: {check}")

    rng = np.random.default_rng(0)
    a = np.cumsum(np.cumsum(rng.integers(-2, 3, (args.batch, args.size, args.size, 3)), axis=1), axis=2).astype(np.float64)
    a -= a.min(axis=(1, 2, 3), keepdims=True)
    imgs = torch.from_numpy((a * 255.0 / np.maximum(a.max(axis=(1, 2, 3), keepdims=True), 1)).astype(np.uint8))

    def step_fn(rate):
        tr = T.Training(device="cuda", weights=W.seeded_weights(0, init="glorot"), seed=0, rate=rate)
        return lambda: tr.train_step(imgs, 0.01)

    steps = {"table": step_fn("table"), "context": step_fn("context")}
    hip_grad = lambda **kw: train_hip.rate_ctable_grad(y, L, anchors, g, groups, seg, yc, **kw)  # noqa: E731
    forms = {
        "forward_hip": (lambda: train_hip.rate_ctable_bits(y, L, anchors, groups, seg, yc), False),
        "forward_torch_fp32": (lambda: T.context_bits(y_nchw, L, anchors, groups, seg, yc_nchw), False),
        "backward_hip_dy_dL": (lambda: hip_grad(), False),
        "backward_hip_dy": (lambda: hip_grad(want_dl=False), False),
        "backward_hip_dL": (lambda: hip_grad(want_dy=False), False),
        "backward_torch_fp32_dy_dL": (back_t, False),
        "train_step_table_events": (steps["table"], False), "train_step_context_events": (steps["context"], False),
        "train_step_table_wall": (steps["table"], True), "train_step_context_wall": (steps["context"], True),
    }
    res = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, (fn, wall) in forms.items():
            res[name].append(round(median_ms(fn, args.iters, args.warmup, wall), 4))
    out = {"tool": "rate_ctable_times", "device": torch.cuda.get_device_name(0), "planes": m, "latent": [hw, hw, c],
           "groups": groups, "seg_pixels": seg, "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds,
           "check": check, "median_ms": res,
           "note": "forward / backward: the loss alone, allocations included; train_step: 64 patches, optimisers "
                   "included, table = the table rate loss (the baseline), context = the context rate loss beside "
                   "the static table's fit"}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
