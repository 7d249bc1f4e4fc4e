"""A CPU model of the f16x3 path's activation split (plain NumPy, no GPU).

The device stores every intermediate activation x as hi = f16(x), lo = f16(x - hi), both rounded
to nearest even, f16 subnormals kept (split4, csrc/nic_kernels.hip); the next layer reads hi + lo.
Here that one step is applied to the float64 oracle's own activations and everything else stays
the oracle's: split_error replaces the chosen sites' activations by hi + lo, runs the real
remaining layers (oracle.nic_oracle._layer, float64 accumulation) and returns the largest change
of the output -- the clipped pre-quant latent of the case's model for the encoder, the clipped
fp32 RGB for the decoder.  It models neither the weights' split nor the fp32 accumulation, so it
is what the activation split alone costs: the yardstick for the low-side cases of
tests/range_sites.py, where a site scaled down by 2^-k is followed by a kernel scaled up by 2^k.
"""
import numpy as np

from oracle import nic_oracle as O
from tests import range_sites as R

F16_MIN_NORMAL = 2.0 ** -14
F16_SUBNORMAL_STEP = 2.0 ** -24


def split(x):
    """(hi, lo) of split4 for fp32 x: hi = f16(x), lo = f16(x - f32(hi)); x - hi is exact in fp32."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def merged(x):
    """hi + lo as the next layer's MFMAs see it (exact in float64)."""
    hi, lo = split(x)
    return hi.astype(np.float64) + lo.astype(np.float64)


def _run(direction, params, plane, sites):
    """encoder_layers / decoder_layers with the activations of `sites` split on the way: the
    residual (conv2 / dconv1) is read back split like any other input, conv4 / dconv6 are split
    after the residual add.  Returns the last layer's output before the clip."""
    enc = direction == "enc"
    names = O.ENCODER_LAYERS if enc else O.DECODER_LAYERS
    strides = (2, 2, 1, 1, 2) if enc else (2, 1, 1, 2, 2)
    res_from, res_into = (1, 3) if enc else (0, 2)
    x, res = plane, None
    for j, name in enumerate(names):
        x = O._layer(x, params, name, strides[j], not enc, np.float64)
        if j == res_into:
            x = x + res
        if name in sites:
            x = merged(x)
        if j == res_from:
            res = x
    return x


def split_error(case, sites):
    """max |delta| of the case's output when the activations of `sites` (one name or several)
    of the case's model are split, against the oracle's output with the same weights."""
    sites = (sites,) if isinstance(sites, str) else tuple(sites)
    assert set(sites) <= set(R.SPLIT_SITES[case.direction])
    kind = "encoder" if case.direction == "enc" else "decoder"
    params = O._model_params(case.weights, kind + case.model)
    planes = O._encoder_planes(case.x) if case.direction == "enc" else O._decoder_planes(case.x)
    ref = O.run_model(case.weights, kind, planes)
    out = list(ref)
    for p in R.PLANES[case.model]:
        out[p] = np.clip(_run(case.direction, params, planes[p], sites).astype(np.float32), 0, 1)
    if case.direction == "dec":
        ref = [np.clip(O.convert_to_rgb(*ref), 0, 1)]
        out = [np.clip(O.convert_to_rgb(*out), 0, 1)]
    return max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(out, ref))


def site_maxima(case):
    """{site: max |activation| over the case's model's planes} in the oracle."""
    acts = case.activations()
    return {s: max(float(np.abs(acts[p][s]).max()) for p in R.PLANES[case.model])
            for s in R.SPLIT_SITES[case.direction]}
