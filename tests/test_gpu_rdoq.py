"""The device side of rate-distortion optimised quantisation (csrc/nic_rdoq.hip: the elementwise
kernel of the static prior and the trellis kernel of the context prior) against the NumPy reference
(tests/rdoq_ref.py), byte for byte: the golden latents and a crafted one at every seg_pixels that
changes the chains' shape, lambda 0 as the identity, the files of the chosen codes through the device
coders, the directory driver, the error paths and the stream contract."""
import os

import numpy as np
import pytest

from tests import rans2_ref as R2
from tests import rans3_ref as R3
from tests import rdoq_ref as Q
from tests import stream_gate as SG

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_image_compression_amd import _lib  # noqa: E402
from neural_network_image_compression_amd import bitstream as B  # noqa: E402
from neural_network_image_compression_amd.codec import Codec, Decoder, Encoder  # noqa: E402
from neural_network_image_compression_amd.prior import ContextPrior, Prior  # noqa: E402

SEG_PIXELS = (1, 5, 32, 64)
LAMS = (0.0, 0.05, 16.0)
CRAFTED_ANCHORS = [0, 255] + [(37 * c + 11) % 256 for c in range(2, 96)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _crafted():
    """A 3 x 5 latent around CRAFTED_ANCHORS (0 and 255 among them) whose pre-quant values are exact
    .5 / 255 ties seen from either side, 0.0, 1.0, one ulp either side of a code, and ordinary ones."""
    rng = np.random.default_rng(3)
    z = np.zeros((1, 3, 5, 96), np.uint8)
    f = np.zeros((1, 3, 5, 96), np.float32)
    for p in range(15):
        for c, a in enumerate(CRAFTED_ANCHORS):
            k = int(np.clip(a + rng.integers(-2, 3), 0, 254))
            kind = (p + c) % 7
            tie = np.float32((k + 0.5) / 255.0)
            at = np.float32(k / 255.0)
            r, v = {0: (k, tie), 1: (k + 1, tie), 2: (0, np.float32(0.0)), 3: (255, np.float32(1.0)),
                    4: (k, np.nextafter(at, np.float32(0.0)) if k else at), 5: (k, np.nextafter(at, np.float32(1.0))),
                    6: (k, np.float32((k + rng.uniform(-0.5, 0.5)) / 255.0))}[kind]
            z[0, p // 5, p % 5, c], f[0, p // 5, p % 5, c] = r, np.clip(v, 0.0, 1.0)
    return z, f


def _crafted_priors():
    rng = np.random.default_rng(4)
    static, rows = [], []
    for a in CRAFTED_ANCHORS:
        w = rng.random((4, 256)) ** 6 + 1e-3
        w[0, a] = 4.0  # the anchor is the static row's argmax
        w[1:, a] += np.array([2.0, 0.5, 0.05])
        f = [R2.normalise_prior((r * 1e6).astype(np.int64)) for r in w]
        static.append(f[0])
        rows.append(f[1:])
    assert R3.anchors_of(static) == CRAFTED_ANCHORS
    return static, (CRAFTED_ANCHORS, rows)


@pytest.fixture(scope="module")
def data(golden):
    """case -> (codes, pre-quant values, static prior, context prior).  odd: the 5 x 7 latent (35 pixels:
    at seg_pixels 32 a full segment and a 3-pixel tail); imagenet4: a batch of 4 of 16 x 16 (at 64, full
    64-pixel chains); both under the priors fitted on the four imagenet4_trained latents."""
    latents = list(golden("imagenet4_trained")["latent"])
    static = R2.fit_prior(latents)
    cprior = R3.fit_context_prior(latents, static)
    odd, im4 = golden("odd37x53"), golden("imagenet4_trained")
    z, f = _crafted()
    cand, D = Q.candidates(z, f)
    moves = cand[..., 1] != cand[..., 0]
    assert (moves & (D[..., 0] == D[..., 1])).sum() >= 20, "the crafted latent holds no exact ties"
    assert (f == 0.0).any() and (f == 1.0).any()
    return {"odd": (odd["latent"], odd["prequant"], static, cprior),
            "imagenet4": (im4["latent"], im4["prequant"], static, cprior),
            "crafted": (z, f) + _crafted_priors()}


@pytest.fixture(scope="module")
def codec():
    c = Codec(0)  # nic_rdoq needs no weights
    yield c
    c.close()


@pytest.fixture()
def primed(codec, data):
    def use(case):
        codec.set_prior(Prior(np.asarray(data[case][2])))
        codec.set_context_prior(ContextPrior(*data[case][3]))
        return codec

    yield use
    codec.set_context_prior(None)
    codec.set_prior(None)


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("case", ["odd", "imagenet4", "crafted"])
def test_device_equals_the_reference(primed, data, case, lam):
    codec = primed(case)
    z, f, static, cprior = data[case]
    zd, fd = _dev(z), _dev(f)
    lam_fix = Q.lam_fix_of(lam)
    got = codec.rdoq(zd, fd, lam, prior="static").cpu().numpy()
    want = Q.rdoq_static(z, f, static, lam_fix)
    print(f"{case} lam {lam}: static moves {100 * np.mean(want != z):.2f} % of the codes")
    np.testing.assert_array_equal(got, want)
    for sp in SEG_PIXELS:
        got = codec.rdoq(zd, fd, lam, seg_pixels=sp).cpu().numpy()  # prior None: the context prior first
        want = Q.rdoq_context(z, f, cprior, lam_fix, sp)
        print(f"{case} lam {lam} seg_pixels {sp}: the trellis moves {100 * np.mean(want != z):.2f} % of the codes")
        np.testing.assert_array_equal(got, want)
        assert np.abs(got.astype(int) - z.astype(int)).max() <= 1
        if lam == 0.0:
            np.testing.assert_array_equal(got, z)
    if lam == 16.0:
        assert (want != z).any()


def test_lambda_zero_returns_the_input_bytes(primed, data):
    codec = primed("imagenet4")
    z, f = _dev(data["imagenet4"][0]), _dev(data["imagenet4"][1])
    for kind in ("static", "context", None):
        out = torch.full_like(z, 7)
        assert codec.rdoq(z, f, 0.0, prior=kind, out=out) is out
        assert SG.same_bytes(out, z)
    # None falls to the static prior when no context prior is set
    codec.set_context_prior(None)
    want = Q.rdoq_static(data["imagenet4"][0], data["imagenet4"][1], data["imagenet4"][2], Q.lam_fix_of(0.05))
    np.testing.assert_array_equal(codec.rdoq(z, f, 0.05).cpu().numpy(), want)
    assert codec.rdoq(z[:0], f[:0], 0.05).shape == (0, 16, 16, 96)  # an empty batch is OK


@pytest.mark.parametrize("case", ["odd", "imagenet4", "crafted"])
def test_the_chosen_codes_round_trip_through_the_device_coders(primed, data, case):
    codec = primed(case)
    z, f = _dev(data[case][0]), _dev(data[case][1])
    n, h8, w8, _ = z.shape
    for sp in (5, 32):
        z3 = codec.rdoq(z, f, 0.05, seg_pixels=sp, prior="context")
        assert SG.same_bytes(codec.rans3_decode(*codec.rans3_encode(z3, sp), h8, w8), z3)
    z2 = codec.rdoq(z, f, 0.05, prior="static")
    assert SG.same_bytes(codec.rans2_decode(*codec.rans2_encode(z2), h8, w8), z2)
    # the device's version-3 file of the device's codes is the reference's file of the reference's codes
    z3 = codec.rdoq(z, f, 0.05, prior="context")
    ref = Q.rdoq_context(data[case][0], data[case][1], data[case][3], Q.lam_fix_of(0.05), 32)
    assert B.nic_files(codec, z3)[0] == R3.write_file(ref[0], data[case][3], 32)


def test_error_paths(codec, primed, data):
    z, f = _dev(data["odd"][0]), _dev(data["odd"][1])
    for kind in ("static", "context", None):
        with pytest.raises(_lib.NicError) as e:
            codec.rdoq(z, f, 0.05, prior=kind)
        assert e.value.code == _lib.NIC_ENOPRIOR
    codec.set_prior(Prior(np.asarray(data["odd"][2])))
    with pytest.raises(_lib.NicError) as e:
        codec.rdoq(z, f, 0.05, prior="context")  # the static prior alone does not serve the trellis
    assert e.value.code == _lib.NIC_ENOPRIOR
    primed("odd")
    for sp in (0, 65):
        with pytest.raises(ValueError, match="1..64"):
            codec.rdoq(z, f, 0.05, seg_pixels=sp)
    for lam in (-0.001, 16.001, float("nan")):
        with pytest.raises(ValueError, match="lam"):
            codec.rdoq(z, f, lam)
    with pytest.raises(ValueError, match="overlaps"):
        codec.rdoq(z, f, 0.05, out=z)
    with pytest.raises(ValueError, match="prior"):
        codec.rdoq(z, f, 0.05, prior="v3")
    with pytest.raises(TypeError):
        codec.rdoq(z, f.double(), 0.05)
    with pytest.raises(TypeError):
        codec.rdoq(z, f[:, :1], 0.05)


def test_compress_with_rdoq_writes_smaller_files_that_uncompress_reads(tmp_path, golden, weights_trained):
    from PIL import Image

    from neural_network_image_compression_amd import weights as W
    g = golden("imagenet4")
    images = {"a0": np.ascontiguousarray(g["x"][0][32:96, 16:80]), "a1": np.ascontiguousarray(g["x"][1][32:96, 16:80]),
              "b_odd": golden("odd37x53")["x"][0], "c0": np.ascontiguousarray(g["x"][2][:61, :50])}
    for d in ("plain", "rdoq"):
        (tmp_path / d).mkdir()
        for name, a in images.items():
            Image.fromarray(np.ascontiguousarray(a)).save(tmp_path / d / f"{name}.png")
    ck = tmp_path / "ck"
    W.save(weights_trained, str(ck / "encoder"), "encoder")
    W.save(weights_trained, str(ck / "decoder"), "decoder")
    enc, dec = Encoder(0), Decoder(0)
    enc.load(str(ck / "encoder"))
    with pytest.raises(ValueError, match="needs a prior"):
        enc.compress(str(tmp_path / "rdoq"), str(ck / "encoder"), container="nic", rdoq=0.05)
    zs = [enc.codec.encode(_dev(np.ascontiguousarray(a)[None])) for a in images.values()]
    acc = Prior.accumulator(enc.codec)
    for z in zs:
        acc.add(z)
    cacc = ContextPrior.accumulator(enc.codec, acc.build())
    for z in zs:
        cacc.add(z)
    cprior = cacc.build()
    with pytest.raises(ValueError, match="container"):
        enc.compress(str(tmp_path / "rdoq"), str(ck / "encoder"), prior=cprior, rdoq=0.05)
    with pytest.raises(ValueError, match="not in"):
        enc.compress(str(tmp_path / "rdoq"), str(ck / "encoder"), container="nic", prior=cprior, rdoq=16.5)
    enc.compress(str(tmp_path / "plain"), str(ck / "encoder"), container="nic", prior=cprior)
    enc.compress(str(tmp_path / "rdoq"), str(ck / "encoder"), container="nic", prior=cprior, rdoq=0.05)
    size = {d: {n: len((tmp_path / f"{d}_compressed" / f"{n}.nic").read_bytes()) for n in images} for d in ("plain", "rdoq")}
    print(f"without rdoq {size['plain']}, with rdoq=0.05 {size['rdoq']}")
    # every file is the device coder's file of encode_rdoq's codes, which differ from encode's by one step at most
    for name, a in images.items():
        x = _dev(np.ascontiguousarray(a)[None])
        want = B.nic_files(enc.codec, enc.encode_rdoq(x, 0.05), size=a.shape[:2])[0]
        assert (tmp_path / "rdoq_compressed" / f"{name}.nic").read_bytes() == want
        assert want[4] == 3
    assert sum(size["rdoq"].values()) < sum(size["plain"].values())
    dec.uncompress(str(tmp_path / "rdoq_compressed"), str(ck / "decoder"), container="nic", prior=cprior)
    out = tmp_path / "rdoq_uncompressed"
    assert sorted(os.listdir(out)) == sorted(n + ".png" for n in images)
    for name, a in images.items():
        with Image.open(out / f"{name}.png") as im:
            assert np.array(im).shape == a.shape


def test_rdoq_runs_on_the_callers_stream_without_a_host_sync(primed, data):
    """Codec.rdoq on a non-default stream, as tests/test_gpu_stream_contract.py builds its cases."""
    codec = primed("imagenet4")
    gate, arena = SG.Gate(0), SG.Arena(0)
    z, f = data["imagenet4"][0], data["imagenet4"][1]
    decoy = np.random.default_rng(8).integers(0, 256, z.shape, dtype=np.uint8)

    def make(which):
        if which == "B":
            return [_dev(z), _dev(f)]
        return [_dev(decoy), _dev((decoy / 255.0).astype(np.float32))]

    for kind, sp in (("context", 5), ("static", 32)):
        got = SG.run_async(gate, arena, f"rdoq-{kind}", make, lambda inp: codec.rdoq(inp[0], inp[1], 0.05, seg_pixels=sp, prior=kind))
        want = Q.rdoq_context(z, f, data["imagenet4"][3], Q.lam_fix_of(0.05), sp) if kind == "context" else \
            Q.rdoq_static(z, f, data["imagenet4"][2], Q.lam_fix_of(0.05))
        np.testing.assert_array_equal(got[0].cpu().numpy(), want)
