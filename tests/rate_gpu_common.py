"""What the GPU tests of the two rate losses share (tests/test_gpu_rate_table.py,
tests/test_gpu_rate_ctable.py): the upstream gradients, the report line, the ulp distance."""
import numpy as np
import torch

G_KINDS = ("equal", "first_group", "signs")


def report(tag, what, *figs):
    print(f"\n[{tag}] {what}: " + " ".join(f"{f:.3e}" if isinstance(f, float) else str(f) for f in figs))


def g(kind, m, groups):
    if kind == "equal":
        return np.full(m, 1.0 / 4096, np.float32)
    if kind == "first_group":  # what loss0 sends down: nothing outside the Y planes
        out = np.zeros(m, np.float32)
        out[:m // groups] = 0.01 / 1024
        return out
    rng = np.random.default_rng(m)
    return (rng.standard_normal(m) * 1e-3).astype(np.float32)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def ulps(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    spacing = torch.ldexp(torch.ones_like(ref), torch.floor(torch.log2(ref.abs().clamp_min(1e-37))).int() - 23)
    return float(((a - ref).abs() / spacing).max())
