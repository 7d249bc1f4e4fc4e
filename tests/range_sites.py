"""Case builders for the f16 range guard, one per split-f16 site (plain NumPy, no GPU).

The f16x3 mode stores every intermediate activation as a pair of f16 halves; a value at or
past 65504 would split into +-inf, so each kernel that writes split activations tracks
max |v| (split_record -> range_track, csrc/nic_kernels.hip) and a tripped pass is re-run in exact fp32.  A case
here is (direction, target site, model, shape, input, weights) such that, in the float64
oracle, the target site reaches at least 2 x 65504 while every other split site of the pass
stays at or below 65504 / 2: only the target site's own range_track can trip the guard, and
if it does not, the pass carries inf / NaN to the output.  tests/test_range_sites.py checks
those conditions for every case; tests/test_gpu_range_sites.py runs the cases on the device.

Every layer is leaky(conv + b), positively homogeneous, and powers of two scale exactly; only
whole layers are scaled (the split-f16 weights share one power-of-two pre-scale per layer, so a
layer with a 2^17 spread between its own weights would lose the small ones' low bits).
"""
import math
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import nic_oracle as O

LIMIT = 65504.0
F32 = np.float32
SPLIT_SITES = {"enc": ("conv1", "conv2", "conv3", "conv4"), "dec": ("dconv1", "dconv5", "dconv6", "dconv7")}
NEXT = {"conv1": "conv2", "conv2": "conv3", "conv3": "conv4", "conv4": "conv8",
        "dconv1": "dconv5", "dconv5": "dconv6", "dconv6": "dconv7", "dconv7": "dconv8"}
PLANES = {"Y": (0,), "CbCr": (1, 2)}


@dataclass
class Case:
    name: str
    direction: str            # "enc" | "dec"
    site: str                 # the split site that must trip
    model: str                # "Y" | "CbCr": the model whose weights are scaled
    shape: Tuple[int, int, int]
    kind: str                 # "exact" | "tied" | "position"
    x: np.ndarray             # u8 image (enc) or u8 latent (dec)
    weights: Dict[str, np.ndarray]
    base: Optional[Dict[str, np.ndarray]] = None   # exact cases: the network whose outputs are unchanged
    fused: bool = True        # the k3 pair runs as one launch (conv3 / dconv5 launch count 0)
    below: bool = False       # k lowered: the target's max lies in [LIMIT / 2, LIMIT), no trip
    cr_only: bool = False     # CbCr: the Cb planes stay at or below LIMIT / 2 at the target too
    share: bool = False       # decoder: the oracle's unclipped share is at least 0.80
    plane: Optional[int] = None      # position cases: 0 Y, 1 Cb, 2 Cr ...
    image: Optional[int] = None      # ... of this image
    centre: Optional[Tuple[int, int]] = None   # chosen pixel in the target layer's plane
    radius: int = 0                  # the target layer's receptive-field radius around it
    cover: List[Tuple[int, int]] = field(default_factory=list)  # pixels that must be over-limit
    low: Optional[int] = None        # low-side cases: the level k, the targets run at 2^-k
    targets: Tuple[str, ...] = ()    # low-side cases: every split site that runs small

    def prefix(self):
        return ("encoder" if self.direction == "enc" else "decoder") + self.model + "/"

    def activations(self, weights=None):
        fn = O.encoder_activations if self.direction == "enc" else O.decoder_activations
        return fn(self.weights if weights is None else weights, self.x)

    def outputs(self, weights=None):
        fn = O.encode_f32 if self.direction == "enc" else O.decode_f32
        return fn(self.weights if weights is None else weights, self.x)


@lru_cache(maxsize=None)
def spread_weights():
    from neural_network_image_compression_amd import weights as W
    w = W.seeded_weights(0, init="spread")
    for v in w.values():
        v.setflags(write=False)
    return w


def seeded_input(direction, shape):
    """The inputs of ENCODE_FORMS / DECODE_FORMS (tests/test_gpu_parity.py): same shapes, same seeds."""
    n, a, b = shape
    rng = np.random.default_rng(1000 * a + b)
    if direction == "enc":
        return rng.integers(0, 256, (n, a, b, 3), dtype=np.uint8)
    return rng.integers(0, 256, (n, a, b, 96), dtype=np.uint8)


def cr_only_input(direction, shape):
    """The seeded input with the Cb planes made small, so that under the shared CbCr weights only
    the Cr planes -- the last planes of the batch -- reach the limit.  Decoder: the Cb codes
    (channels 32..63) >> 4.  Encoder: near-yellow pixels (R, G in 230..255, B in 0..7), Cb <= 0.07
    against Cr ~ 0.53."""
    x = seeded_input(direction, shape).copy()
    if direction == "dec":
        x[..., 32:64] >>= 4
    else:
        x[..., 0] = 230 + x[..., 0] % 26
        x[..., 1] = 230 + x[..., 1] % 26
        x[..., 2] = x[..., 2] % 8
    return x


def k_over(m):
    """Smallest k with m * 2^k >= 2 * LIMIT (1.001: room for the residual a tied site adds)."""
    return int(math.ceil(math.log2(2.002 * LIMIT / float(m))))


def k_below(m):
    """Largest k with m * 2^k < LIMIT (then >= LIMIT / 2); 0.999 keeps it strictly below."""
    return int(math.floor(math.log2(0.999 * LIMIT / float(m))))


def _scale(w, key, s):
    w[key] = (w[key] * F32(s)).astype(F32)


def _scale_layer(w, pre, site, k):
    """site's kernel and bias x 2^k, the next layer's kernel x 2^-k."""
    _scale(w, pre + site + "/kernel", 2.0 ** k)
    _scale(w, pre + site + "/bias", 2.0 ** k)
    _scale(w, pre + NEXT[site] + "/kernel", 2.0 ** -k)


def _own(acts, site):
    """What the site's own layer adds: conv4 / dconv6 without the residual."""
    res = {"conv4": "conv2", "dconv6": "dconv1"}.get(site)
    return acts[site] if res is None else acts[site] - acts[res]


def scaled_site(direction, site, model, shape, fused, below=False, cr_only=False):
    """conv1, conv3, dconv5, dconv7 (kind "exact"): the layer's kernel and bias x 2^k and the
    next layer's kernel x 2^-k leave the oracle's outputs unchanged bit for bit (what
    range_scaled_weights does for conv3 / dconv5).  conv4, dconv6 (kind "tied"): the same scaling
    of conv4 and conv8 (dconv6 and dconv7) gives 2^k leaky(conv4) + a2, over the limit, while a2
    (conv2 / dconv1) keeps its size: another network, its outputs 2^-k a2 away from the original's,
    evaluated live.  k comes from the oracle's own activations of the target planes (Cr for
    CbCr); with `below` it is the largest k that keeps the target under the limit."""
    assert site in ("conv1", "conv3", "conv4", "dconv5", "dconv6", "dconv7")
    base = spread_weights()
    x = cr_only_input(direction, shape) if cr_only else seeded_input(direction, shape)
    c = Case(f"{site}-{model}-{'x'.join(map(str, shape))}" + ("-below" if below else ""), direction, site, model,
             shape, "tied" if site in ("conv4", "dconv6") else "exact", x, dict(base), fused=fused, below=below,
             cr_only=cr_only)
    acts = c.activations()
    m = max(float(np.abs(_own(acts[p], site)).max()) for p in PLANES[model][-1:])
    _scale_layer(c.weights, c.prefix(), site, k_below(m) if below else k_over(m))
    if c.kind == "exact":
        c.base = base
    return c


def first_of_tied(direction, model, shape, fused):
    """conv2 alone (dconv1 alone), kind "tied".  The residual carries conv2's output a2 into
    conv4 + res, so a2 over the limit puts that site over it too -- unless conv4 takes it back.
    Construction (whole layers only): conv2's bias becomes the constant B = 16 r in every channel,
    r = max |conv2's sum| on this input, so a2' = conv + B lies in [15 r, 17 r], positive and
    narrow; conv2 x 2^k (max in [2, 4) x LIMIT) and conv3's kernel x 2^-k; conv4 gets a zero
    kernel and the bias -5 mid_c per channel (leaky: -mid_c), mid_c the middle of that channel's
    range, so conv4 + res = a2 - mid_c, within r 2^k < 4/15 LIMIT; conv8's kernel x 2^-k brings
    the latent back into (0, 1).  The latent still depends on every a2 value, so a stale plane
    after the re-run shows.  The decoder's dconv1 / dconv5 / dconv6 / dconv7 alike."""
    L = ("conv2", "conv3", "conv4", "conv8") if direction == "enc" else ("dconv1", "dconv5", "dconv6", "dconv7")
    c = Case(f"{L[0]}-{model}-{'x'.join(map(str, shape))}", direction, L[0], model, shape, "tied",
             seeded_input(direction, shape), dict(spread_weights()), fused=fused)
    w, pre = c.weights, c.prefix()
    w[pre + L[0] + "/bias"] = np.zeros_like(w[pre + L[0] + "/bias"])
    a = np.concatenate([c.activations()[p][L[0]] for p in PLANES[model]])
    r = float(np.abs(np.where(a < 0, a / 0.2, a)).max())  # the sum before leaky
    w[pre + L[0] + "/bias"] = np.full_like(w[pre + L[0] + "/bias"], 16 * r)
    a = np.concatenate([c.activations()[p][L[0]] for p in PLANES[model]])
    assert a.min() > 0
    k = k_over(float(a.max()))
    _scale_layer(w, pre, L[0], k)
    a = np.concatenate([c.activations()[p][L[0]] for p in PLANES[model]]).astype(np.float64)
    mid = 0.5 * (a.max(axis=(0, 1, 2)) + a.min(axis=(0, 1, 2)))
    w[pre + L[2] + "/kernel"] = np.zeros_like(w[pre + L[2] + "/kernel"])
    w[pre + L[2] + "/bias"] = (-5.0 * mid).astype(F32)
    _scale(w, pre + L[3] + "/kernel", 2.0 ** -k)
    return c


def _zero_biases(w, pre, layers):
    for name in layers:
        w[pre + name + "/bias"] = np.zeros_like(w[pre + name + "/bias"])


def decoder_position(site, shape, pix8, cover, fused, name):
    """One non-zero latent pixel `pix8` = (y8, x8) in the Cr channels of the last image, zero
    biases in the CbCr model up to and including the target: every CbCr activation up to the
    target is exactly zero outside that pixel's receptive field.  The target is scaled as in
    scaled_site, k chosen so that every pixel of `cover` (target plane coordinates) is over
    2 x LIMIT.  Receptive field in the target plane: dconv1 rows 2 y8 - 1 .. 2 y8 + 3 (centre
    2 y8 + 1, radius 2), one more per k3 layer, dconv7 centre 4 y8 + 3, radius 10.
    dconv1 as the target also has to keep dconv6 + res = a2 + ... in range where a2 is a few
    isolated large values, which no bias can re-centre: there dconv1's kernel is |kernel| x 2^k
    (the latent is >= 0, so a2 >= 0), dconv5 is the identity x 2^-k (centre tap only), dconv6 the
    centre tap -5 x 2^k, whose leaky is -a2: dconv6 + res cancels to rounding level.  What is
    left is the rounding of values near 2^18 (about 0.03, and not the same in two correct fp32
    evaluations), so dconv7's kernel is x 2^-k as well and the Cb / Cr output is dconv7's and
    dconv8's biases: this one case checks the trip, the error and the re-run's identity with
    the fp32 codec, not a non-trivial output."""
    n, h8, w8 = shape
    order = ("dconv1", "dconv5", "dconv6", "dconv7")
    z = np.zeros((n, h8, w8, 96), np.uint8)
    z[n - 1, pix8[0], pix8[1], 64:] = np.random.default_rng(7).integers(128, 256, 32, dtype=np.uint8)
    c = Case(name, "dec", site, "CbCr", shape, "position", z, dict(spread_weights()), fused=fused, plane=2,
             image=n - 1)
    w, pre = c.weights, c.prefix()
    _zero_biases(w, pre, order[:order.index(site) + 1])
    if site == "dconv7":
        c.centre, c.radius = (4 * pix8[0] + 3, 4 * pix8[1] + 3), 10
    else:
        c.centre, c.radius = (2 * pix8[0] + 1, 2 * pix8[1] + 1), 2 + order.index(site)
    c.cover = list(cover)
    if site == "dconv1":
        w[pre + "dconv1/kernel"] = np.abs(w[pre + "dconv1/kernel"])
    a = _own(c.activations()[2], site)[n - 1]
    k = k_over(min(float(np.abs(a[y, x]).max()) for y, x in cover))
    if site == "dconv1":
        _scale(w, pre + "dconv1/kernel", 2.0 ** k)
        eye = np.zeros_like(w[pre + "dconv5/kernel"])
        eye[1, 1] = np.eye(64, dtype=F32)
        w[pre + "dconv5/kernel"] = eye * F32(2.0 ** -k)
        w[pre + "dconv6/kernel"] = eye * F32(-5.0 * 2.0 ** k)
        _zero_biases(w, pre, ("dconv5", "dconv6"))
        _scale(w, pre + "dconv7/kernel", 2.0 ** -k)
    else:
        _scale_layer(w, pre, site, k)
    return c


def encoder_position_conv1(shape):
    """conv12's conv1 site at the last row and column of an odd-sized plane: a black image
    (Y = 0) with a white 3 x 3 patch in the bottom right corner of the last image, conv1's bias
    zero in the Y model, conv1 x 2^k and conv2's kernel x 2^-k.  conv1 (k5, s2, odd size: rows
    2 oy - 2 .. 2 oy + 2) is non-zero only within 2 of its last pixel.  (The Cb and Cr planes of
    an image cannot both be zero, and a plane that is not makes the shared CbCr weights overflow
    everywhere, so the encoder's position case is a Y plane; the decoder's are Cr.)"""
    n, h, wd = shape
    assert h % 2 and wd % 2
    x = np.zeros((n, h, wd, 3), np.uint8)
    x[n - 1, h - 3:, wd - 3:] = 255
    c = Case("conv1-last-pixel", "enc", "conv1", "Y", shape, "position", x, dict(spread_weights()), plane=0,
             image=n - 1)
    _zero_biases(c.weights, c.prefix(), ("conv1",))
    oh, ow = (h + 1) // 2, (wd + 1) // 2
    c.centre, c.radius, c.cover = (oh - 1, ow - 1), 2, [(oh - 1, ow - 1)]
    a = c.activations()[0]["conv1"][n - 1]
    _scale_layer(c.weights, c.prefix(), "conv1", k_over(float(np.abs(a[oh - 1, ow - 1]).max())))
    return c


# encoder shapes: the pair at MT=3, the two-launch form, the strip pair with a short last strip;
# decoder: the pair at MT=2, the two-launch form, the strip pair (ENCODE_FORMS / DECODE_FORMS)
E_PAIR, E_WS, E_STRIP = (2, 24, 130), (1, 24, 257), (2, 24, 469)
D_PAIR, D_WS, D_STRIP, D_ROWS = (2, 3, 9), (1, 3, 33), (2, 3, 59), (1, 40, 2)


@lru_cache(maxsize=None)
def site_cases():
    """Every row of the split-site table, each k3 site in its three forms, the models
    alternating so that each kernel trips under both."""
    S, T = scaled_site, first_of_tied
    cases = [
        S("enc", "conv1", "CbCr", E_PAIR, True, cr_only=True),
        T("enc", "Y", E_STRIP, True),
        S("enc", "conv3", "Y", E_PAIR, True), S("enc", "conv3", "CbCr", E_WS, False, cr_only=True),
        S("enc", "conv3", "CbCr", E_STRIP, True, cr_only=True),
        S("enc", "conv4", "CbCr", E_PAIR, True, cr_only=True), S("enc", "conv4", "Y", E_WS, False),
        S("enc", "conv4", "Y", E_STRIP, True),
        T("dec", "Y", D_PAIR, True),
        S("dec", "dconv5", "CbCr", D_PAIR, True, cr_only=True), S("dec", "dconv5", "Y", D_WS, False),
        S("dec", "dconv5", "Y", D_STRIP, True),
        S("dec", "dconv6", "Y", D_PAIR, True), S("dec", "dconv6", "CbCr", D_WS, False, cr_only=True),
        S("dec", "dconv6", "CbCr", D_STRIP, True, cr_only=True),
        S("dec", "dconv7", "Y", D_PAIR, True),
    ]
    for c in cases:  # the share bound holds on the unchanged inputs of DECODE_FORMS
        c.share = c.direction == "dec" and c.kind == "exact" and not c.cr_only
    return cases


@lru_cache(maxsize=None)
def position_cases():
    """One per kernel: over-limit values only around the last row and column of the last plane
    of the last image (conv12: of the last Y plane); the strip pair also at its seam columns 61 /
    62; the pair also in an 80-row plane cut into many block ranges (240 rows over 60 blocks of
    about 4: the over-limit conv_a rows 38 .. 44 span more than one range, so at least one of
    them is a row that a range boundary recomputes)."""
    P = decoder_position
    return [
        encoder_position_conv1((2, 21, 131)),
        P("dconv1", D_PAIR, (2, 8), [(5, 17)], True, "dconv1-last-pixel"),
        P("dconv5", D_PAIR, (2, 8), [(5, 17)], True, "pair-a-last-pixel"),
        P("dconv6", D_PAIR, (2, 8), [(5, 17)], True, "pair-b-last-pixel"),
        P("dconv5", D_ROWS, (20, 1), [(y, 3) for y in range(38, 45)], True, "pair-a-range-boundary"),
        P("dconv6", D_STRIP, (2, 58), [(5, 117)], True, "strip-b-last-pixel"),
        P("dconv5", D_STRIP, (2, 58), [(5, 117)], True, "strip-a-last-pixel"),
        P("dconv5", D_STRIP, (1, 30), [(3, 61), (3, 62)], True, "strip-a-seam"),
        P("dconv6", D_STRIP, (1, 30), [(3, 61), (3, 62)], True, "strip-b-seam"),
        P("dconv5", D_WS, (2, 32), [(5, 65)], False, "ws-a-last-pixel"),
        P("dconv6", D_WS, (2, 32), [(5, 65)], False, "ws-b-last-pixel"),
        P("dconv7", D_PAIR, (2, 8), [(11, 35)], True, "dconv7-last-pixel"),
    ]


@lru_cache(maxsize=None)
def below_cases():
    """The same construction with k lowered: the target's max in [LIMIT / 2, LIMIT), no trip."""
    return [scaled_site("enc", "conv3", "Y", E_PAIR, True, below=True),
            scaled_site("dec", "dconv7", "CbCr", D_PAIR, True, below=True)]


def all_cases():
    return site_cases() + position_cases() + below_cases()


# ---- the low side of the f16 range -----------------------------------------------------------
# lo = f16(x - f16(x)) is about 2^-11 |x|: below 2^-14 it is an f16 subnormal with the fixed
# spacing 2^-24, so a site whose activations run at 2^-k carries an absolute split error of up to
# 2^-25 whatever k is, and the next layer's kernel, larger by 2^k, multiplies it back up.  The
# cases scale whole layers down by exact powers of two and compensate downstream: the float64
# oracle's outputs are those of the unscaled spread network bit for bit (tests/test_range_sites.py),
# the high-side guard is nowhere near, and tests/split_f16_model.py predicts what the split loses.
LOW_LEVELS = (4, 8, 12, 17, 24)  # 24: hi itself is flushed to zero for typical values
LOW_SINGLE = {"enc": ("conv1", "conv3"), "dec": ("dconv5", "dconv7")}
TRUNK = {"enc": ("conv2", "conv3", "conv4", "conv8"), "dec": ("dconv1", "dconv5", "dconv6", "dconv7")}
# (shape, fused): the smallest of ENCODE_FORMS / DECODE_FORMS that take the fused pair (the
# decoder's with the Y -> CbCr switch inside a block) and the two-launch form
LOW_SHAPES = {"enc": ((E_PAIR, True), (E_WS, False)), "dec": (((2, 3, 8), True), (D_WS, False))}


def _low_case(direction, what, targets, model, shape, fused, k):
    base = spread_weights()
    c = Case(f"low-{what}-{model}-{'x'.join(map(str, shape))}-k{k}", direction, targets[0], model, shape, "exact",
             seeded_input(direction, shape), dict(base), base=base, fused=fused, low=k, targets=tuple(targets))
    c.share = direction == "dec"  # DECODE_FORMS' own inputs, the unscaled network's outputs
    return c


def low_site(direction, site, model, shape, fused, k):
    """scaled_site's mirror: the site's kernel and bias x 2^-k, the next layer's kernel x 2^k."""
    assert site in LOW_SINGLE[direction]
    c = _low_case(direction, site, (site,), model, shape, fused, k)
    _scale_layer(c.weights, c.prefix(), site, -k)
    return c


def low_trunk(direction, model, shape, fused, k):
    """conv2's kernel and bias, conv3's bias and conv4's bias x 2^-k, conv8's kernel x 2^k: conv2,
    conv3 and conv4 + res all run at 2^-k and the network is unchanged (conv3's and conv4's kernels
    see inputs that are already small).  The only exact way to put the residual sites conv2 and
    conv4 (dconv1 and dconv6: the decoder's dconv1 / dconv5 / dconv6 / dconv7 alike) on the low
    side: the residual ties their scales together."""
    L = TRUNK[direction]
    c = _low_case(direction, "trunk", L[:3], model, shape, fused, k)
    w, pre = c.weights, c.prefix()
    _scale(w, pre + L[0] + "/kernel", 2.0 ** -k)
    for name in L[:3]:
        _scale(w, pre + name + "/bias", 2.0 ** -k)
    _scale(w, pre + L[3] + "/kernel", 2.0 ** k)
    return c


@lru_cache(maxsize=None)
def low_cases(levels=LOW_LEVELS):
    """Every single site and the whole trunk, under the Y and the CbCr model, in the fused and the
    two-launch form, at every level.  No level had to be dropped: nothing underflows in fp32 and
    the bit-identity holds up to k = 24 (tests/test_range_sites.py)."""
    out = []
    for direction in ("enc", "dec"):
        for shape, fused in LOW_SHAPES[direction]:
            for model in ("Y", "CbCr"):
                for k in levels:
                    for site in LOW_SINGLE[direction]:
                        out.append(low_site(direction, site, model, shape, fused, k))
                    out.append(low_trunk(direction, model, shape, fused, k))
    return out


def child_cases():
    """The two site cases outside the k3 pair that tests/range_guard_check.py runs under the
    re-run's load-time switches: conv2 and dconv7."""
    return [c for c in site_cases() if c.site in ("conv2", "dconv7")]
