"""A NumPy float64 restatement of nic_resample_boxes (include/nic.h): the antialiased bilinear resize of
torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=True), the flip, and
the three output kinds.  Test infrastructure only: plain loops over the output indices, dense weight
matrices, no attempt at speed."""
import numpy as np

EPS = 2.0 ** -23


def axis_weights(n_in: int, n_out: int):
    """(W (n_out, n_in) float64 with each row's normalised tap weights, taps (n_out,) int: the tap counts)."""
    s = n_in / n_out
    support = max(s, 1.0)
    inv = 1.0 / max(s, 1.0)
    W = np.zeros((n_out, n_in), np.float64)
    taps = np.zeros(n_out, np.int64)
    for i in range(n_out):
        c = s * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        cnt = min(int(c + support + 0.5), n_in) - lo
        w = np.array([max(0.0, 1.0 - abs((j + lo - c + 0.5) * inv)) for j in range(cnt)], np.float64)
        W[i, lo:lo + cnt] = w / w.sum()
        taps[i] = cnt
    return W, taps


def resize(box, size, flip=False):
    """box (bh, bw, 3) of values 0..255 -> ((oh, ow, 3) float64 in the same units, Ty (oh,), Tx (ow,))."""
    box = np.asarray(box, np.float64)
    Wy, Ty = axis_weights(box.shape[0], size[0])
    Wx, Tx = axis_weights(box.shape[1], size[1])
    out = np.einsum("ikc,lk->ilc", np.tensordot(Wy, box, axes=(1, 0)), Wx)  # rows first, then columns
    if flip:
        out, Tx = out[:, ::-1], Tx[::-1]
    return np.ascontiguousarray(out), Ty, np.ascontiguousarray(Tx)


def scale_bias(mean, std):
    """What Codec.resample_boxes hands the kernel: float64 arithmetic, rounded to fp32."""
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def crop(image, row, size, kind, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """One table row (oy, ox, bh, bw, flip[, dst]) of image (Hs, Ws, 3) u8.
    kind "float32" / "float16": ((3, oh, ow) float64 = v scale + bias, its tolerance);
    kind "uint8": ((oh, ow, 3) float64, not rounded, in 0..255 units, its tolerance: 0.5 is in it)."""
    oy, ox, bh, bw, flip = (int(v) for v in row[:5])
    v, Ty, Tx = resize(image[oy:oy + bh, ox:ox + bw], size, bool(flip))
    taps = (4 + Ty[:, None] + Tx[None, :]).astype(np.float64)
    if kind == "uint8":
        v = np.clip(v, 0.0, 255.0)
        return v, 0.5 + taps[:, :, None] * EPS * 255.0 + EPS * np.abs(v)
    scale, bias = scale_bias(mean, std)
    ref = (v * scale.astype(np.float64) + bias.astype(np.float64)).transpose(2, 0, 1)
    tol = taps[None] * EPS / np.abs(np.asarray(std, np.float64))[:, None, None] + EPS * np.abs(ref)
    if kind == "float16":
        tol = tol + 2.0 ** -11 * np.abs(ref)
    return ref, tol


def rounded_u8(v):
    """The u8 kind's value: half to even, clamped."""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)
