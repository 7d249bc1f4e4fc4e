"""include/nic.h's stream contract, held per entry point: "work is enqueued asynchronously on the
caller's hipStream_t", "on `stream`, no host synchronisation", "everything runs on `stream`".

Every other GPU test runs on the default stream and synchronises, where a launch, memset or copy
given stream 0, a host synchronisation hidden in a call and an allocation in a warm call all give
the same bytes.  Here each call runs on a torch side stream (non-blocking: the null stream does not
wait for it) behind a gate that holds the stream, with its inputs copied in behind the gate and
every buffer it allocates pre-filled with a sentinel (tests/stream_gate.py):

  test_on_stream_no_host_sync   CASES: the call returns while the gate is pending, nothing it
                                allocated is written while the gate is pending, and its outputs
                                equal the default-stream results byte for byte
  test_documented_sync_waits    SYNC_CASES: the calls that synchronise by their own words do not
                                return before the gate ends, and still give the right results
  test_one_ctx_two_streams...   one ctx on two streams that the caller orders (nic.h conventions)

Shapes are the smallest that keep each call a chain of kernels: images (2, 24, 40, 3), latents
(2, 3, 5, 96), .nic files at seg_pixels 4 (four segments), training planes (2, 16, 24) (the
MS-SSIM loss at (2, 1, 22, 26): two scales need 11 pixels at the second), gather g5, wgrad w5, the
rate shape (2, 3, 3, 24, 2).  Gate calibration and the warm host time of every case: printed by
each case (-s), recorded in DESIGN.md section 24.
"""
import zlib

import numpy as np
import pytest

from tests import rate_table_ref as RT
from tests import stream_gate as SG
from tests import train_ref as R

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IMG = (2, 24, 40, 3)
LAT = (2, 3, 5, 96)
BIG = (2, 161, 163, 3)  # nic_ms_ssim: every one of its five scales holds the 11 x 11 window
SEG = 4
PLANES = (2, 16, 24)
MS_PLANES = (2, 1, 22, 26)
RATE = (2, 3, 3, 24, 2)  # (M, h, w, C, G): rate_table_ref.SHAPES' entry with R = 64 // C = 2
assert RATE in RT.SHAPES
G5 = next(c for c in R.GATHER_CASES if c.id == "g5")
W5 = next(c for c in R.WGRAD_CASES if c.id == "w5")
PNG_STRIDE = 4096


def _seed(which, salt=0):
    return torch.Generator().manual_seed({"A": 11, "B": 23}[which] * 1000 + salt)


def _img(which, shape=IMG, salt=0):
    """A ramp with noise, stronger in B than in A: compressible, so PNG and .nic sizes differ."""
    n, h, w, c = shape
    ramp = (torch.arange(h)[:, None, None] * 3 + torch.arange(w)[None, :, None] * 2 + torch.arange(c)[None, None, :] * 40) % 256
    noise = torch.randn(shape, generator=_seed(which, salt)) * {"A": 4.0, "B": 14.0}[which]
    return (ramp[None].float() + noise).clamp(0, 255).to(torch.uint8).to(DEV)


def _lat(which, salt=0):
    z = torch.randn(LAT, generator=_seed(which, 50 + salt)) * {"A": 6.0, "B": 17.0}[which] + 128
    return z.clamp(0, 255).to(torch.uint8).to(DEV)


def _f32(which, shape, salt=0, lo=-1.0, hi=1.0):
    return (torch.rand(shape, generator=_seed(which, 100 + salt)) * (hi - lo) + lo).to(DEV)


def _ints(which, shape, hi, dtype, salt=0):
    return torch.randint(0, hi, shape, generator=_seed(which, 200 + salt)).to(dtype).to(DEV)


def _canon(buf, sizes):
    """Files with the bytes behind their sizes zeroed: those are never written."""
    keep = torch.arange(buf.shape[1], device=buf.device)[None, :] < sizes[:, None]
    return torch.where(keep, buf, torch.zeros_like(buf))


def _u8(shape):
    return torch.empty(shape, dtype=torch.uint8, device=DEV)


class Env:
    def __init__(self, weights):
        from neural_network_image_compression_amd import prior as P
        from neural_network_image_compression_amd.codec import Codec
        from tests.test_gpu_parity import range_scaled_weights

        self.gate = SG.Gate(0)
        self.arena = SG.Arena(0)
        print(f"[stream-contract] gate calibration: {self.gate.cycles_per_ms:.0f} _sleep cycles per ms")
        self.codecs = {}
        for prec in ("f16x3", "fp32"):
            self.codecs[prec] = c = Codec(0, precision=prec)
            c.set_weights(weights)
        scaled = range_scaled_weights(weights)
        self.trip = Codec(0)
        self.trip.set_weights(scaled)
        self.trip32 = Codec(0, precision="fp32")
        self.trip32.set_weights(scaled)
        rng = np.random.default_rng(5)
        self.priors, self.cpriors = [], []
        for _ in range(2):
            p = np.exp(2.0 * rng.standard_normal((96, 256)))
            pr = P.from_probabilities(p / p.sum(axis=1, keepdims=True))
            q = np.exp(2.0 * rng.standard_normal((96, 3, 256)))
            self.priors.append(pr)
            self.cpriors.append(P.context_from_probabilities(P.anchors_of(pr), q / q.sum(axis=2, keepdims=True)))
        assert self.priors[0].id != self.priors[1].id and self.cpriors[0].id != self.cpriors[1].id
        c = self.codecs["f16x3"]
        c.set_prior(self.priors[0])
        c.set_context_prior(self.cpriors[0])

    @property
    def c(self):
        return self.codecs["f16x3"]


@pytest.fixture(scope="module")
def env(weights_spread):
    return Env(weights_spread)


# ---- the catalogue: name -> builder(env) -> (make, call, reserve or None[, post]) ------------------
CASES = {}


def case(name):
    def add(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return add


def _encode_case(prec, prequant):
    def build(e):
        c = e.codecs[prec]
        return (lambda w: [_img(w)],
                lambda inp: c.encode(inp[0], prequant=prequant, out=_u8(LAT)),
                lambda: c.reserve(*IMG[:3]))
    return build


def _decode_case(prec, rgb_f32):
    def build(e):
        c = e.codecs[prec]
        return (lambda w: [_lat(w)],
                lambda inp: c.decode(inp[0], rgb_f32=rgb_f32, out=_u8(IMG)),
                lambda: c.reserve(*IMG[:3]))
    return build


for _prec in ("f16x3", "fp32"):
    for _flag in (False, True):
        CASES[f"encode-{_prec}" + ("-prequant" if _flag else "")] = _encode_case(_prec, _flag)
        CASES[f"decode-{_prec}" + ("-rgb_f32" if _flag else "")] = _decode_case(_prec, _flag)


def _encode_entropy_case(counts):
    def build(e):
        return (lambda w: [_img(w)],
                lambda inp: e.c.encode_entropy(inp[0], counts=counts, out=_u8(LAT)),
                lambda: e.c.reserve(*IMG[:3]))
    return build


CASES["encode_entropy"] = _encode_entropy_case(False)
CASES["encode_entropy-counts"] = _encode_entropy_case(True)

# At IMG the latent is one conv8 tile per plane and nic_encode_entropy runs its two-call form (nic_encode,
# then nic_entropy_hist).  Its own chain -- conv8 counting the codes into the ctx's fold_acc, then
# launch_hist_fold, which clears what it read for the next call -- needs every block to meet a plane
# in two tiles: (h8 + 3) // 4 * ((w8 + 7) // 8) >= 342 tiles per plane on 256 CUs.  One frame of
# 640 x 1216 has 20 x 19 = 380.  fold_acc is state that one call leaves for the next, so the decoy's
# counts are what a piece of the call that ran early, or did not clear, would show.
FOLD_IMG = (1, 640, 1216, 3)
FOLD_LAT = (1, 80, 152, 96)


def _encode_entropy_fold_case(counts):
    def build(e):
        assert e.c.encode_entropy_folds(*FOLD_IMG[:3]), "this shape no longer takes the folded form on this device"
        return (lambda w: [_img(w, FOLD_IMG)],
                lambda inp: e.c.encode_entropy(inp[0], counts=counts, out=_u8(FOLD_LAT)),
                lambda: e.c.reserve(*FOLD_IMG[:3]))
    return build


CASES["encode_entropy-fold"] = _encode_entropy_fold_case(False)
CASES["encode_entropy-fold-counts"] = _encode_entropy_fold_case(True)


@case("entropy")
def _(e):
    return (lambda w: [_lat(w)], lambda inp: e.c.entropy(inp[0], counts=True), lambda: e.c.reserve(*IMG[:3]))


@case("ms_ssim-per_scale")
def _(e):
    return (lambda w: [_img(w, BIG), _img(w, BIG, salt=1)], lambda inp: e.c.ms_ssim(inp[0], inp[1], per_scale=True), None)


@case("sq_err")
def _(e):
    return (lambda w: [_img(w), _img(w, salt=1)], lambda inp: e.c.sq_err(inp[0], inp[1]), None)


@case("pack")
def _(e):
    return (lambda w: [_lat(w)], lambda inp: e.c.pack(inp[0]), None)


@case("unpack")
def _(e):
    return (lambda w: [_img(w, (2, 12, 40, 3))], lambda inp: e.c.unpack(inp[0]), None)


# -- the .nic coders --
_RANS = {1: "rans", 2: "rans2", 3: "rans3"}


def _files(e, ver, which):
    """Clean files of B; the decoy's second file is cut inside its header, so its status differs too."""
    buf, sizes = getattr(e.c, _RANS[ver] + "_encode")(_lat(which), SEG)
    buf = _canon(buf, sizes)
    if which == "A":
        sizes[1] = 10
    return [buf, sizes]


def _rans_reserve(e, ver):
    return lambda: getattr(e.c, _RANS[ver] + "_reserve")(LAT[0], LAT[1], LAT[2], SEG)


def _rans_encode_case(ver):
    def build(e):
        def call(inp):
            buf, sizes = getattr(e.c, _RANS[ver] + "_encode")(inp[0], SEG)
            return _canon(buf, sizes), sizes
        return (lambda w: [_lat(w)], call, _rans_reserve(e, ver))
    return build


def _rans_decode_case(ver):
    def build(e):
        return (lambda w: _files(e, ver, w),
                lambda inp: getattr(e.c, _RANS[ver] + "_decode_status")(inp[0], inp[1], LAT[1], LAT[2], out=_u8(LAT)),
                _rans_reserve(e, ver))
    return build


WINDOW = (1, 1, 2, 3)  # r0, c0, rows, cols: pixels of segments 1, 2 and 3, not of segment 0
WINDOWS = {"A": [[3, 5, 1, 0], [3, 5, 0, 2]], "B": [[3, 5, 0, 1], [3, 5, 1, 2]]}  # h8, w8, r0, c0 per file


def _rans_window_case(ver):
    def build(e):
        return (lambda w: _files(e, ver, w),
                lambda inp: getattr(e.c, _RANS[ver] + "_decode_window_status")(inp[0], inp[1], LAT[1], LAT[2], WINDOW,
                                                                              out=_u8((2, 2, 3, 96))),
                _rans_reserve(e, ver))
    return build


def _rans_windows_case(ver):
    def build(e):
        return (lambda w: _files(e, ver, w) + [torch.tensor(WINDOWS[w], dtype=torch.int32).to(DEV)],
                lambda inp: getattr(e.c, _RANS[ver] + "_decode_windows_status")(inp[0], inp[1], inp[2], (2, 3), max_pixels=15,
                                                                               out=_u8((2, 2, 3, 96))),
                _rans_reserve(e, ver))
    return build


for _ver in (1, 2, 3):
    CASES[_RANS[_ver] + "_encode"] = _rans_encode_case(_ver)
    CASES[_RANS[_ver] + "_decode_status"] = _rans_decode_case(_ver)
    CASES[_RANS[_ver] + "_decode_window_status"] = _rans_window_case(_ver)
    CASES[_RANS[_ver] + "_decode_windows_status-device_table"] = _rans_windows_case(_ver)


@case("prior_count")
def _(e):
    def call(inp):
        e.c.prior_count(inp[0], inp[1])
        return inp[1]
    return (lambda w: [_lat(w), _ints(w, (96, 256), 1000, torch.int64)], call, None)


@case("prior_build")
def _(e):
    return (lambda w: [_ints(w, (96, 256), 5000, torch.int64)], lambda inp: e.c.prior_build(inp[0]), None)


@case("cprior_count")
def _(e):
    def call(inp):
        e.c.cprior_count(inp[0], inp[1], inp[2], SEG)
        return inp[2]
    return (lambda w: [_lat(w), _ints(w, (96,), 256, torch.uint8, 1), _ints(w, (96, 3, 256), 1000, torch.int64, 2)], call, None)


@case("cprior_build")
def _(e):
    return (lambda w: [_ints(w, (96, 3, 256), 5000, torch.int64)], lambda inp: e.c.cprior_build(inp[0]), None)


# -- boxes, resampling, PNG --
@case("cut_boxes-device_table")
def _(e):
    offs = {"A": [[3, 7], [16, 0]], "B": [[0, 28], [9, 13]]}
    return (lambda w: [_img(w), torch.tensor(offs[w], dtype=torch.int32).to(DEV)],
            lambda inp: e.c.cut_boxes(inp[0], inp[1], 8, 12, out=_u8((2, 8, 12, 3))), None)


BOX_ROWS = {"A": [[1, 1, 10, 12, 1, 1], [3, 2, 18, 25, 0, 0]], "B": [[2, 3, 16, 20, 0, 0], [0, 5, 20, 30, 1, 1]]}
NORM = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def _resample_out(dtype):
    return torch.empty((2, 8, 10, 3) if dtype == torch.uint8 else (2, 3, 8, 10), dtype=dtype, device=DEV)


def _resample_boxes_case(dtype):
    def build(e):
        return (lambda w: [_img(w), torch.tensor(BOX_ROWS[w], dtype=torch.int32).to(DEV)],
                lambda inp: e.c.resample_boxes(inp[0], inp[1], (8, 10), dtype=dtype, out=_resample_out(dtype), **NORM), None)
    return build


POOL_ROWS = {"A": [[0, 10, 14, 1, 2, 8, 9, 1 | 1 << 32], [432, 12, 9, 0, 0, 12, 9, 0]],
             "B": [[0, 10, 14, 0, 0, 10, 14, 0], [432, 12, 9, 1, 1, 10, 8, 1 | 1 << 32]]}  # (10,14,3) at 0, (12,9,3) at 432


def _resample_pool_case(dtype):
    def build(e):
        return (lambda w: [_ints(w, (756,), 256, torch.uint8, 3), torch.tensor(POOL_ROWS[w], dtype=torch.int64).to(DEV)],
                lambda inp: e.c.resample_pool(inp[0], inp[1], (8, 10), dtype=dtype, out=_resample_out(dtype), **NORM), None)
    return build


for _name, _dtype in (("float32", torch.float32), ("uint8", torch.uint8)):
    CASES["resample_boxes-device_table-" + _name] = _resample_boxes_case(_dtype)
    CASES["resample_pool-" + _name] = _resample_pool_case(_dtype)


@case("png_encode")
def _(e):
    def call(inp):
        buf, sizes = e.c.png_encode(inp[0])
        return _canon(buf, sizes), sizes
    return (lambda w: [_img(w)], call, lambda: e.c.png_reserve(*IMG))


def _zlib_streams(which):
    """Filter-0 zlib streams of the images (dynamic blocks with matches); the decoy's second is cut to
    one byte, so its status differs."""
    x = _img(which).cpu().numpy()
    buf = np.zeros((IMG[0], PNG_STRIDE), np.uint8)
    sizes = np.zeros(IMG[0], np.int64)
    for i, im in enumerate(x):
        s = zlib.compress(b"".join(b"\x00" + row.tobytes() for row in im), 6)
        assert len(s) <= PNG_STRIDE
        buf[i, :len(s)] = np.frombuffer(s, np.uint8)
        sizes[i] = len(s)
    if which == "A":
        sizes[1] = 1
    return [torch.from_numpy(buf).to(DEV), torch.from_numpy(sizes).to(DEV)]


@case("png_read_status")
def _(e):
    return (_zlib_streams, lambda inp: e.c.png_read_status(inp[0], inp[1], IMG[1], IMG[2], IMG[3], out=_u8(IMG)),
            lambda: e.c.png_read_reserve(*IMG))


# -- train_hip --
def _th():
    from neural_network_image_compression_amd import train_hip
    return train_hip


def _gather_case(act):
    def build(e):
        g = G5
        return (lambda w: [_f32(w, (g.n, g.h, g.w, g.cin)), _f32(w, (g.kh, g.kw, g.cin, g.cout), 1), _f32(w, (g.cout,), 2)],
                lambda inp: _th().gather(inp[0], inp[1], g.layout, g.stride, g.pad, g.transposed, g.out_hw, g.cout, inp[2], act=act),
                None)
    return build


CASES["conv_gather-g5-absmax_scale"] = _gather_case(0)
CASES["conv_gather_act-g5-absmax_scale"] = _gather_case(1)


@case("act_bias_grad")
def _(e):
    shape = (G5.n, *G5.out_hw, G5.cout)
    amp = {"A": 16.0, "B": 1.0}  # another power of two of max |dz|, so dz_scale differs too
    return (lambda w: [_f32(w, shape), _f32(w, shape, 1) * amp[w]], lambda inp: _th().act_bias_grad(inp[0], inp[1], 1), None)


@case("conv_wgrad-w5-absmax_scale")
def _(e):
    c = W5
    return (lambda w: [_f32(w, (c.n, *c.gat_hw, c.ca)), _f32(w, (c.n, c.uh, c.uw, c.cb), 1)],
            lambda inp: _th().wgrad(inp[0], inp[1], c.kh, c.kw, c.stride, c.pad), None)


def _gauss_case(vertical, adjoint):
    def build(e):
        return (lambda w: [_f32(w, PLANES), _f32(w, (11,), 1, 0.0, 0.2)],
                lambda inp: _th().gauss_1d(inp[0], inp[1], vertical, adjoint), None)
    return build


CASES["gauss_1d"] = _gauss_case(0, 0)
CASES["gauss_1d-adjoint"] = _gauss_case(1, 1)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _terms(w):
    mx, my = _f32(w, PLANES, 0, 0.0, 1.0), _f32(w, PLANES, 1, 0.0, 1.0)
    return [mx, my, mx * my + _f32(w, PLANES, 2, 0.0, 0.05), mx * mx + my * my + _f32(w, PLANES, 3, 0.1, 0.2)]


@case("msssim_terms")
def _(e):
    return (_terms, lambda inp: _th().msssim_terms(*inp, C1, C2), None)


@case("msssim_terms_grad")
def _(e):
    return (lambda w: _terms(w) + [_f32(w, (PLANES[0],), 4), _f32(w, (PLANES[0],), 5)],
            lambda inp: _th().msssim_terms_grad(*inp, C1, C2), None)


@case("pool2_prep")
def _(e):
    return (lambda w: [_f32(w, PLANES, 0, 0.0, 1.0), _f32(w, PLANES, 1, 0.0, 1.0)], lambda inp: _th().pool2_prep(inp[0], inp[1]), None)


@case("pool2_prep_grad")
def _(e):
    half = (PLANES[0], PLANES[1] // 2, PLANES[2] // 2)
    return (lambda w: [_f32(w, half, i) for i in range(6)], lambda inp: _th().pool2_prep_grad(*inp, PLANES[1:]), None)


@case("ms_ssim_mean")
def _(e):
    return (lambda w: [_f32(w, MS_PLANES, 0, 0.0, 1.0), _f32(w, MS_PLANES, 1, 0.0, 1.0)],
            lambda inp: _th().ms_ssim_mean(inp[0], inp[1], 2), None)


@case("ms_ssim_mean-backward")
def _(e):
    def call(inp):
        x, y = inp[0].detach().requires_grad_(), inp[1].detach().requires_grad_()
        v = _th().ms_ssim_mean(x, y, 2)
        gx, gy = torch.autograd.grad(v, (x, y), inp[2])
        return v.detach(), gx, gy
    return (lambda w: [_f32(w, MS_PLANES, 0, 0.0, 1.0), _f32(w, MS_PLANES, 1, 0.0, 1.0), _f32(w, (MS_PLANES[0],), 2, 0.5, 1.5)], call, None)


def _rate_inputs(contexts, with_g, with_yc):
    m, h, w_, c, groups = RATE

    def make(w):
        rng = np.random.default_rng({"A": 3, "B": 4}[w])
        logits = 2.0 * rng.standard_normal((groups * c * contexts, 256))
        L = torch.from_numpy(RT.code_lengths(logits).astype(np.float32)).to(DEV)
        inp = [_f32(w, (m, h, w_, c), 0, 0.0, 1.0), L if contexts == 1 else L.view(groups * c, 3, 256)]
        if contexts == 3:
            inp.append(_ints(w, (groups * c,), 256, torch.uint8, 1))
        if with_g:
            inp.append(_f32(w, (m,), 2, 0.5, 1.5))
        if with_yc:
            inp.append(_f32(w, (m, h, w_, c), 3, 0.0, 1.0))
        return inp
    return make


@case("rate_table_bits")
def _(e):
    return (_rate_inputs(1, False, False), lambda inp: _th().rate_table_bits(inp[0], inp[1], RATE[4]), None)


@case("rate_table_grad")
def _(e):
    return (_rate_inputs(1, True, False), lambda inp: _th().rate_table_grad(inp[0], inp[1], inp[2], RATE[4]), None)


def _ctable_case(grad, with_yc):
    def build(e):
        def call(inp):
            yc = inp[-1] if with_yc else None
            if grad:
                return _th().rate_ctable_grad(inp[0], inp[1], inp[2], inp[3], RATE[4], SEG, yc=yc)
            return _th().rate_ctable_bits(inp[0], inp[1], inp[2], RATE[4], SEG, yc=yc)
        return (_rate_inputs(3, grad, with_yc), call, None)
    return build


for _grad in (False, True):
    for _yc in (False, True):
        CASES["rate_ctable_" + ("grad" if _grad else "bits") + ("-yc" if _yc else "")] = _ctable_case(_grad, _yc)


@case("keras_adam_step")
def _(e):
    """inputs: two parameters, their m and v slots and gradients; the optimiser of a parameter pair is
    kept, so the gated step is its third and waits on the (long finished) event of its second."""
    shapes = [(7, 5), (33,)]
    opts = {}

    def call(inp):
        p, m, v, g = inp[0:2], inp[2:4], inp[4:6], inp[6:8]
        key = p[0].data_ptr()
        if key not in opts:
            with e.arena.paused():
                opts[key] = _th().KerasAdam(p)
        opt = opts[key]
        for i in range(2):
            opt.m[i].copy_(m[i])
            opt.v[i].copy_(v[i])
        opt.iterations = 2
        opt.step(g)
        return (*p, *opt.m, *opt.v)

    def make(w):
        return ([_f32(w, s, i) for i, s in enumerate(shapes)] + [_f32(w, s, 2 + i, -0.1, 0.1) for i, s in enumerate(shapes)]
                + [_f32(w, s, 4 + i, 0.0, 0.01) for i, s in enumerate(shapes)] + [_f32(w, s, 6 + i) for i, s in enumerate(shapes)])
    return (make, call, None)


@case("range_fallback_trip")
def _(e):
    """A split-f16 pass that trips the f16 range guard under NIC_RANGE_FALLBACK: the gated exact-fp32
    re-run follows on the same stream and rewrites every output, so the bytes are the exact-fp32 ones."""
    c, state = e.trip, {}

    def call(inp):
        return c.encode(inp[0], prequant=True, out=_u8(LAT))

    def make(w):
        x = _img(w)
        if w == "B":
            state["before"] = c.range_trips()
            state["fp32"] = [t.clone() for t in e.trip32.encode(x, prequant=True)]
        return [x]

    def post(got):
        assert SG.same_bytes(got[0], state["fp32"][0]) and SG.same_bytes(got[1], state["fp32"][1]), \
            "the gated call's bytes are not the exact-fp32 pass's"
        x = _img("B")
        z, f = c.encode(x, prequant=True)
        trips = c.range_trips()  # synchronises
        assert trips - state["before"] == 6, "every encode of these weights trips: A, B, two warm runs, the gated one, this one"
        assert SG.same_bytes(z, state["fp32"][0]) and SG.same_bytes(f, state["fp32"][1]), "the re-run's bytes are not the exact-fp32 pass's"
        assert e.trip32.range_trips() == 0
    return (make, call, lambda: c.reserve(*IMG[:3]), post)


# Outputs that torch computes, in stream order, from buffers of the sentinel arena, and that therefore
# lie outside it (stream_gate.run_async): the masked file buffer of the encoders, prior_build's int32
# conversion, the MS-SSIM loss's torch-side combination and autograd's sums, the optimiser's own slots.
OUTSIDE = {"rans_encode": 1, "rans2_encode": 1, "rans3_encode": 1, "png_encode": 1, "prior_build": 1, "cprior_build": 1,
           "ms_ssim_mean": 1, "ms_ssim_mean-backward": 3, "keras_adam_step": 4}
assert set(OUTSIDE) <= set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_on_stream_no_host_sync(env, name):
    make, call, reserve, *post = CASES[name](env)
    got = SG.run_async(env.gate, env.arena, name, make, call, reserve, outside=OUTSIDE.get(name, 0))
    for fn in post:
        fn(got)


# ---- the calls that synchronise by their own words -------------------------------------------------
SYNC_CASES = {}


def sync_case(name):
    def add(fn):
        assert name in SG.SYNCHRONISING_GATED and name not in SYNC_CASES
        SYNC_CASES[name] = fn
        return fn
    return add


def _live(src_a):
    """An input buffer that holds the decoy until the gated stream copies B into it."""
    t = src_a.clone()
    torch.cuda.synchronize()
    return t


@sync_case("encode_host")
def _(e):
    x = _img("B")
    want = e.c.encode(x).cpu().numpy()
    host = x.cpu().numpy()
    return dict(call=lambda: e.c.encode_host(host, 3), check=lambda z: np.testing.assert_array_equal(z, want))


@sync_case("decode_host")
def _(e):
    z = _lat("B")
    want = e.c.decode(z).cpu().numpy()
    host = z.cpu().numpy()
    return dict(call=lambda: e.c.decode_host(host, 3), check=lambda x: np.testing.assert_array_equal(x, want))


def _set_prior_case(ver):
    def build(e):
        old, new = (e.priors, e.cpriors)[ver - 2]
        setter = (e.c.set_prior, e.c.set_context_prior)[ver - 2]
        encode = getattr(e.c, _RANS[ver] + "_encode")
        buf, sizes = encode(_lat("B"), SEG)
        want = [_canon(buf, sizes).clone(), sizes.clone()]
        z, got = _live(_lat("A")), {}

        def setup():
            z.copy_(_lat_b)
            got["files"] = encode(z, SEG)  # queued behind the gate: reads the old prior when the gate ends

        def check(_):
            try:
                buf, sizes = got["files"]
                assert SG.same_bytes(sizes, want[1]) and SG.same_bytes(_canon(buf, sizes), want[0]), \
                    "files queued before the new prior was set were not coded under the old one"
                buf2, sizes2 = encode(_lat_b, SEG)
                assert not SG.same_bytes(_canon(buf2, sizes2), want[0]), "the new prior codes the same files: the case cannot tell"
            finally:
                setter(old)
        _lat_b = _lat("B")
        return dict(setup=setup, call=lambda: setter(new), check=check, warm=False)
    return build


SYNC_CASES["set_prior"] = _set_prior_case(2)
SYNC_CASES["set_context_prior"] = _set_prior_case(3)


@sync_case("range_trips")
def _(e):
    before = e.trip.range_trips()
    x, xb = _live(_img("A")), _img("B")

    def setup():
        x.copy_(xb)
        e.trip.encode(x)
    return dict(setup=setup, call=e.trip.range_trips, check=lambda n: n == before + 1 or pytest.fail(f"{n} trips, expected {before + 1}"),
                warm=False)


@sync_case("layer_times")
def _(e):
    x, xb = _live(_img("A")), _img("B")

    def setup():
        x.copy_(xb)
        e.c.set_timing(True)  # nothing pending yet: does not wait
        e.c.encode(x)

    def check(t):
        e.c.set_timing(False)
        assert t["conv2"][1] == 1 and t["conv8"][1] == 1 and t["conv2"][0] > 0 and t["conv8"][0] > 0, t
    return dict(setup=setup, call=e.c.layer_times, check=check, warm=False)


@sync_case("encode_range_error")
def _(e):
    xb = _img("B")
    want = e.c.encode(xb).clone()
    x = _live(_img("A"))

    def call():
        e.c.set_range_policy("error")
        try:
            return e.c.encode(x)
        finally:
            e.c.set_range_policy("fallback")
    return dict(setup=lambda: x.copy_(xb), call=call, check=lambda z: SG.same_bytes(z, want) or pytest.fail("wrong latent"), warm=False)


@pytest.mark.parametrize("name", list(SG.SYNCHRONISING_GATED))
def test_documented_sync_waits(env, name):
    SG.run_sync(env.gate, name, **SYNC_CASES[name](env))


def test_synchronising_list_quotes_the_sources():
    """Every wrapper kept out of the gate stands in the helper with the words of nic.h or of its
    docstring that say it synchronises, and those words are in the sources."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = ""
    for path in (("include", "nic.h"), ("neural_network_image_compression_amd", "codec.py")):
        with open(os.path.join(root, *path)) as f:
            text += " " + f.read()
    text = " ".join(text.replace("*", " ").split())
    for text_of in ("returns with the outputs written (synchronous)", "Synchronous (waits for the device)",
                    "nic_range_trips (synchronising)", "Both synchronise on the recorded events",
                    "the call synchronises its stream after the split pass"):
        assert text_of in text, text_of
    for table in (SG.SYNCHRONISING_UNGATED, SG.SYNCHRONISING_FOUND):
        for who, fragments in table.items():
            assert fragments, who
            for frag in fragments:
                assert " ".join(frag.split()) in text, (who, frag)
    assert set(SYNC_CASES) == set(SG.SYNCHRONISING_GATED)


def test_one_ctx_two_streams_ordered_by_caller(env):
    """nic.h conventions: one ctx may be used on several streams of one thread when the caller orders
    its calls across them (the workspace and the range word are the ctx's, not the stream's).  encode on
    stream 1, then decode on stream 2 after wait_stream, both behind gates: neither call waits on the
    host, nothing runs early, both results are the default-stream ones."""
    e, g = env, env.gate
    c = e.c
    xb, zb = _img("B"), _lat("B")
    want_z, want_x = c.encode(xb).clone(), c.decode(zb).clone()
    x, z = _live(_img("A")), _live(_lat("A"))
    c.reserve(*IMG[:3])
    s1, s2 = g.side, g.other
    for _ in range(2):  # warm, on the streams the gated calls use
        with torch.cuda.stream(s1):
            c.encode(x)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            c.decode(z)
        torch.cuda.synchronize()
    e.arena.reset()
    torch.cuda.synchronize()
    ev1 = g.hold(s1, SG.GATE_MIN_MS)
    with e.arena.open():
        with torch.cuda.stream(s1):
            x.copy_(xb)
            got_z = c.encode(x, out=_u8(LAT))
        s2.wait_stream(s1)
        ev2 = g.hold(s2, SG.GATE_MIN_MS / 4)
        with torch.cuda.stream(s2):
            z.copy_(zb)
            got_x = c.decode(z, out=_u8(IMG))
    early = not ev1.query() and not ev2.query()
    clean = e.arena.untouched(g.third)
    held = not ev1.query()
    torch.cuda.synchronize()
    assert early, "a call on the ordered streams waited on the host"
    assert held, "gate too short"
    assert clean, "an output was written while stream 1 was still held"
    assert SG.same_bytes(got_z, want_z) and SG.same_bytes(got_x, want_x)
