"""Device time of a rate loss on HIP beside its PyTorch restatement, and what it costs the training
step, in one process, at the training shape: 192 planes of 16 x 16 x 32 (a batch of 64 patches of
128 x 128), 3 groups.  --rate table: the table rate loss (nic_rate_table, training.table_bits),
the step beside rate "png" (the Entropynet and the host PNG target).  --rate context: the context
rate loss (nic_rate_ctable, training.context_bits; segments of --seg-pixels), the step beside rate
"table" (the baseline).

  forward      the HIP loss alone (train_hip.rate_[c]table_bits) against the restatement on the same
               device tensors (NCHW, as backend="torch" holds them)
  backward     the HIP gradient call with both gradients, dy alone and dL alone, against the
               restatement's autograd backward (both gradients; its forward is not in the figure)
  train_step   Training.train_step on 64 patches, backend "hip", with the baseline rate and with
               --rate, alternating; wall-clock per step with a device synchronisation at its end,
               beside the hipEvent figure

hipEvents on the current stream, the median of `--iters` calls after `--warmup`, `--rounds` such
medians per form with the forms alternating (all reported).  Before timing, the HIP loss and both
gradients are checked against the restatement (1e-4 of the largest reference value).

Output: one JSON line, also written to --out (profiles/rate_table_times.json or
profiles/rate_ctable_times.json).  Needs the GPU and the built library."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, iters, warmup, wall=False):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 if wall else a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", choices=("table", "context"), required=True)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--seg-pixels", type=int, default=32, help="--rate context only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from neural_network_image_compression_amd import train_hip
    from neural_network_image_compression_amd import training as T
    from neural_network_image_compression_amd import weights as W

    context = args.rate == "context"
    tool = "rate_ctable_times" if context else "rate_table_times"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", tool + ".json")
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: needs the GPU")
    groups, c, seg = T.TABLE_GROUPS, T.TABLE_CHANNELS, args.seg_pixels
    m, hw = groups * args.batch, args.size // 8
    gen = torch.Generator().manual_seed(0)
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()  # noqa: E731
    # a latent like the step's: a third of it clamped at 0, the rest spread
    y = (torch.rand((m, hw, hw, c), generator=gen) * 1.5 - 0.5).clamp(0, 1)
    if context:  # the contexts come from the clean latent, the rate is taken at the noisy one
        yc = y.cuda()
        y = (y + (torch.rand(y.shape, generator=gen) - 0.5) / 255).clamp(0, 1).cuda()
        L = T.context_code_lengths(torch.randn((groups * c, 3, 256), generator=gen).cuda()).contiguous()
        anchors = torch.randint(0, 4, (groups * c,), generator=gen, dtype=torch.uint8).cuda()
        y_nchw, yc_nchw = nchw(y), nchw(yc)
        torch_bits = lambda yy, LL: T.context_bits(yy, LL, anchors, groups, seg, yc_nchw)  # noqa: E731
        hip_bits = lambda: train_hip.rate_ctable_bits(y, L, anchors, groups, seg, yc)  # noqa: E731
        hip_grad = lambda **kw: train_hip.rate_ctable_grad(y, L, anchors, g, groups, seg, yc, **kw)  # noqa: E731
    else:
        y = y.cuda()
        L = T.table_code_lengths(torch.randn((groups * c, 256), generator=gen).cuda()).contiguous()
        y_nchw = nchw(y)
        torch_bits = lambda yy, LL: T.table_bits(yy, LL, groups)  # noqa: E731
        hip_bits = lambda: train_hip.rate_table_bits(y, L, groups)  # noqa: E731
        hip_grad = lambda **kw: train_hip.rate_table_grad(y, L, g, groups, **kw)  # noqa: E731
    g = torch.full((m,), 1.0 / (m * args.size * args.size), device="cuda")

    def torch_backward():
        yy, LL = y_nchw.detach().requires_grad_(), L.detach().requires_grad_()
        bits = torch_bits(yy, LL)
        return bits, lambda: torch.autograd.grad((bits * g).sum(), (yy, LL), retain_graph=True)

    bits_t, back_t = torch_backward()
    dy_t, dl_t = back_t()
    bits_h = hip_bits()
    dy_h, dl_h = hip_grad()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    check = {"bits_rel": rel(bits_h, bits_t.detach()), "dy_rel": rel(dy_h, dy_t.permute(0, 2, 3, 1)),
             "dL_rel": rel(dl_h, dl_t)}
    if max(check.values()) > 1e-4:
        raise SystemExit(f"{tool}: the HIP loss differs from the restatement: {check}")

    rng = np.random.default_rng(0)
    a = np.cumsum(np.cumsum(rng.integers(-2, 3, (args.batch, args.size, args.size, 3)), axis=1), axis=2).astype(np.float64)
    a -= a.min(axis=(1, 2, 3), keepdims=True)
    imgs = torch.from_numpy((a * 255.0 / np.maximum(a.max(axis=(1, 2, 3), keepdims=True), 1)).astype(np.uint8))

    def step_fn(rate):
        tr = T.Training(device="cuda", weights=W.seeded_weights(0, init="glorot"), seed=0, rate=rate)
        return lambda: tr.train_step(imgs, 0.01)

    rates = ("table", "context") if context else ("png", "table")  # the baseline, then --rate
    steps = {rate: step_fn(rate) for rate in rates}
    forms = {
        "forward_hip": (hip_bits, False),
        "forward_torch_fp32": (lambda: torch_bits(y_nchw, L), False),
        "backward_hip_dy_dL": (lambda: hip_grad(), False),
        "backward_hip_dy": (lambda: hip_grad(want_dl=False), False),
        "backward_hip_dL": (lambda: hip_grad(want_dy=False), False),
        "backward_torch_fp32_dy_dL": (back_t, False),
    }
    forms.update({f"train_step_{rate}_events": (steps[rate], False) for rate in rates})
    forms.update({f"train_step_{rate}_wall": (steps[rate], True) for rate in rates})
    res = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, (fn, wall) in forms.items():
            res[name].append(round(median_ms(fn, args.iters, args.warmup, wall), 4))
    out = {"tool": tool, "device": torch.cuda.get_device_name(0), "planes": m, "latent": [hw, hw, c], "groups": groups}
    if context:
        out["seg_pixels"] = seg
    out.update({"iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "check": check, "median_ms": res,
                "note": "forward / backward: the loss alone, allocations included; train_step: 64 patches, optimisers "
                        "included, " + ("table = the table rate loss (the baseline), context = the context rate loss "
                                        "beside the static table's fit" if context else
                                        "png = Entropynet + host PNG target (16 threads), table = the table rate loss")})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
