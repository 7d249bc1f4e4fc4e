"""Host-side mirror of the reference codec surface, running on the HIP C-ABI.

Reference classes (AlexFuster/Neural_network_image_compression, tf2_0/src):

* ``ProClass`` (utils.py:15-62): owns the Y and CbCr models, ``load(path)`` reads
  ``path + 'Y'`` and ``path + 'CbCr'``, ``_use_model``/``_feed_batch`` drive directories.
* ``Encoder`` (encoder.py:34-51): ``__call__(x)`` u8 (N,H,W,3) -> u8 (N,h,w,96);
  ``compress(dataset_path, checkpoint_path)``.
* ``Decoder`` (decoder.py:35-52): ``__call__(z)`` u8 (N,h,w,96) -> u8 (N,8h,8w,3);
  ``uncompress(dataset_path, checkpoint_path)``.

Here the per-plane Keras models become one fused device pipeline over all 3N planes
(``libnic.so``).  ``__call__`` accepts NumPy arrays (copied to and from the device, like
the reference's ``.numpy()`` hand-offs) or ROCm ``torch.uint8`` tensors (no host copy;
work is queued on the current torch stream and a device tensor is returned).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np

from . import _lib
from . import weights as W


def _torch():
    import torch

    return torch


def _stream_ptr(torch, device: int) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _as_u8_array(x, what: str) -> np.ndarray:
    a = np.asarray(x)
    if a.dtype == np.uint8:
        return a
    if a.dtype.kind in "iuf":
        # the reference computes x.astype(float32)/255 (encoder.py:39, decoder.py:40); the
        # device path is defined on u8 codes, so only exactly representable inputs are taken
        if a.size and (not np.all(np.isfinite(a)) or np.any(a != np.round(a)) or a.min() < 0 or a.max() > 255):
            raise ValueError(f"{what}: values must be integers in [0, 255], got dtype {a.dtype}")
        return a.astype(np.uint8)
    raise TypeError(f"{what}: unsupported dtype {a.dtype}")


FIT_MODES = ("stretch", "center", "shorter")
POOL_ALIGN = 16  # bytes: every image of a pool starts at a multiple of it (nic_resample_ragged needs 4)


def fit_boxes(shapes, size, mode: str = "center") -> np.ndarray:
    """The box (oy, ox, bh, bw) of every (H, W) of shapes that a resize to size = (oh, ow) reads: an
    (N, 4) int64 array, rows for Codec.resample_ragged.  Integer arithmetic throughout.

    "stretch": the whole image, (0, 0, H, W); the resize changes the aspect ratio.
    "center":  the largest centred box with the output's aspect ratio.  One side is the image's own:
               where W oh >= H ow (the image is at least as wide as the output) bh = H and
                   bw = max(1, (2 H ow + oh) // (2 oh)),
               which is H ow / oh rounded to the nearest integer, halves up, and never above W; else
               bw = W and bh = max(1, (2 W oh + ow) // (2 ow)).  Among the boxes with that full side
               no other width has bw / bh nearer to ow / oh (no other height bh / bw nearer to
               oh / ow), and where W oh == H ow the box is the whole image.  oy = (H - bh) // 2 and ox = (W - bw) // 2, so the box's centre is the
               image's or half a pixel before it.
    "shorter": "center" under the name of torchvision's Resize(shorter side) + CenterCrop, which is
               what it stands for.  The two differ in one thing: torchvision first resizes the whole
               image to an integer size (the longer side rounded) and then cuts oh x ow output pixels
               out of it, so its crop edges fall on output pixels; here the box's edges fall on source
               pixels and the box is resized once.  The source region differs by less than one output
               pixel's footprint per side, and the single resize does not filter twice.

    ValueError for a shape or size that is not two integers >= 1, or another mode."""
    if mode not in FIT_MODES:
        raise ValueError(f"fit_boxes: mode must be one of {FIT_MODES}, got {mode!r}")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"fit_boxes: size must be (oh, ow), got {size!r}") from None
    hw = np.asarray(shapes, dtype=np.int64).reshape(-1, 2) if len(shapes) else np.zeros((0, 2), np.int64)
    if oh < 1 or ow < 1 or (hw.size and hw.min() < 1):
        raise ValueError("fit_boxes: shapes and size must be integers >= 1")
    H, W = hw[:, 0], hw[:, 1]
    if mode == "stretch":
        bh, bw = H.copy(), W.copy()
    else:
        wide = W * oh >= H * ow
        bw = np.where(wide, np.maximum(1, (2 * H * ow + oh) // (2 * oh)), W)
        bh = np.where(wide, H, np.maximum(1, (2 * W * oh + ow) // (2 * ow)))
    return np.stack([(H - bh) // 2, (W - bw) // 2, bh, bw], axis=1)


def pool_layout(shapes):
    """Where tightly packed (H, W, 3) u8 images of the (H, W) of shapes go in one pool: (their byte
    offsets, each a multiple of POOL_ALIGN, in order and as close as that allows; the pool's size,
    which ends on the last image's last byte)."""
    offsets, at, end = [], 0, 0
    for h, w in shapes:
        offsets.append(at)
        end = at + 3 * int(h) * int(w)
        at = -(-end // POOL_ALIGN) * POOL_ALIGN
    return offsets, end


def pack_images(images, pool: Optional[np.ndarray] = None):
    """Host (H, W, 3) u8 arrays of any sizes -> (pool, offsets): image i's bytes, rows tight, are
    pool[offsets[i] : offsets[i] + 3 H W] (pool_layout).  pool: the u8 array to fill (at least the
    layout's size; page-locked for an asynchronous upload), default a new one; the padding between
    images is left as it was.  ValueError naming the image that is not (H, W, 3) u8 with H, W >= 1."""
    arrays = []
    for i, a in enumerate(images):
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"pack_images: image {i}: expected an (H, W, 3) uint8 array with H, W >= 1, got {a.dtype} {a.shape}")
        arrays.append(a)
    offsets, total = pool_layout([a.shape[:2] for a in arrays])
    if pool is None:
        pool = np.zeros(total, np.uint8)
    elif pool.dtype != np.uint8 or pool.ndim != 1 or pool.size < total or not pool.flags.c_contiguous:
        raise ValueError(f"pack_images: pool must be a contiguous 1-D uint8 array of at least {total} bytes")
    for a, off in zip(arrays, offsets):
        pool[off:off + a.size].reshape(a.shape)[...] = a
    return pool, offsets


class Codec:
    """One ``nic_ctx`` on one HIP device: weights + workspace for encode/decode/entropy."""

    def __init__(self, device: Optional[int] = None, precision: str = "f16x3"):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("neural_network_image_compression_amd needs a ROCm GPU (no CPU fallback)")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._L.nic_create(self.device, ctypes.byref(h)), "nic_create")
        self._h = h
        self._keep: Dict[str, np.ndarray] = {}
        self.precision = precision

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.nic_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights ---------------------------------------------------------------------
    def set_tensor(self, model: str, layer: str, kind: str, value: np.ndarray) -> None:
        a = np.ascontiguousarray(value, dtype=np.float32)
        shape = (ctypes.c_int64 * a.ndim)(*a.shape)
        rc = self._L.nic_set_weights(self._h, W.MODEL_ID[model], f"{layer}/{kind}".encode(), a.ctypes.data,
                                     shape, a.ndim)
        _lib.check(rc, f"nic_set_weights({model}/{layer}/{kind})")

    def set_weights(self, weights: W.Weights) -> None:
        """Uploads the tensors.  Every model that `weights` holds completely first gets its small
        split-f16 sites lifted by exact powers of two (weights.lift_low_sites: the same function,
        bit for bit in fp32; a no-op for weights of ordinary scale), so that the f16x3 path does
        not lose a down-scaled layer in f16 subnormals.  set_tensor uploads as given."""
        for key, value in W.lift_low_sites(weights).items():
            model, layer, kind = key.split("/")
            if model not in W.MODEL_ID:
                raise KeyError(f"unknown model {model!r} in key {key!r}")
            self.set_tensor(model, layer, kind, value)

    def ready(self):
        e, d = ctypes.c_int(), ctypes.c_int()
        _lib.check(self._L.nic_weights_ready(self._h, ctypes.byref(e), ctypes.byref(d)), "nic_weights_ready")
        return bool(e.value), bool(d.value)

    @property
    def precision(self) -> str:
        m = ctypes.c_int()
        _lib.check(self._L.nic_get_precision(self._h, ctypes.byref(m)), "nic_get_precision")
        return {v: k for k, v in _lib.PRECISIONS.items()}[m.value]

    @precision.setter
    def precision(self, mode: str) -> None:
        """'f16x3' (default: split-f16 MFMA) or 'fp32' (exact fp32 MFMA) for the Cin>=32 convs."""
        if mode not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {mode!r}")
        _lib.check(self._L.nic_set_precision(self._h, _lib.PRECISIONS[mode]), "nic_set_precision")

    def set_range_policy(self, policy: str) -> None:
        """f16 range guard of the split-f16 mode (include/nic.h NIC_RANGE_*): 'fallback'
        (default; a tripped pass is recomputed by the exact-fp32 kernels on the device) or
        'error' (the call synchronises and raises NicError(NIC_ERANGE))."""
        if policy not in _lib.RANGE_POLICIES:
            raise ValueError(f"range policy must be one of {sorted(_lib.RANGE_POLICIES)}, got {policy!r}")
        _lib.check(self._L.nic_set_range_policy(self._h, _lib.RANGE_POLICIES[policy]), "nic_set_range_policy")

    def range_trips(self) -> int:
        """Encode/decode passes whose split-f16 activations left the f16 range (synchronises)."""
        n = ctypes.c_int64()
        _lib.check(self._L.nic_range_trips(self._h, ctypes.byref(n)), "nic_range_trips")
        return int(n.value)

    def rerun_launch_info(self) -> dict:
        """How the chained exact-fp32 re-run launches here (nic_rerun_launch_info)."""
        v = [ctypes.c_int() for _ in range(3)]
        _lib.check(self._L.nic_rerun_launch_info(self._h, *[ctypes.byref(t) for t in v]), "nic_rerun_launch_info")
        return {"blocks_per_cu": v[0].value, "grid": v[1].value, "cooperative": bool(v[2].value)}

    def decode_launch_info(self, n: int, h8: int, w8: int) -> dict:
        """The grids the f16x3 decode of (n, h8, w8, 96) latents launches here
        (nic_decode_launch_info): dconv1's and dconv7's blocks for (Y, CbCr), the fused
        dconv5+dconv6 pair's grid (0: two launches)."""
        v = (ctypes.c_int * 5)()
        _lib.check(self._L.nic_decode_launch_info(self._h, n, h8, w8, v), "nic_decode_launch_info")
        return {"dconv1": (v[0], v[1]), "dconv7": (v[2], v[3]), "pair": v[4]}

    def set_timing(self, enable: bool) -> None:
        """Bracket every layer launch with hipEvents on the launch stream (resets the sums)."""
        _lib.check(self._L.nic_set_timing(self._h, int(bool(enable))), "nic_set_timing")

    def layer_times(self):
        """{layer: (total_ms, launches)} accumulated since set_timing(True)."""
        ms = np.zeros(len(_lib.LAYER_NAMES), np.float64)
        cnt = np.zeros(len(_lib.LAYER_NAMES), np.int64)
        _lib.check(self._L.nic_layer_times(self._h, ms.ctypes.data, cnt.ctypes.data), "nic_layer_times")
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(_lib.LAYER_NAMES)}

    def reserve(self, n: int, h: int, w: int) -> None:
        _lib.check(self._L.nic_reserve(self._h, n, h, w), "nic_reserve")

    # -- device entry points (torch uint8 tensors on this device) ----------------------
    def _check_dev(self, t, ndim: int, last: int, what: str):
        torch = _torch()
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device.type != "cuda":
            raise TypeError(f"{what}: expected a cuda torch.uint8 tensor")
        if t.device.index != self.device:
            raise ValueError(f"{what}: tensor on cuda:{t.device.index}, codec on cuda:{self.device}")
        if t.ndim != ndim or t.shape[-1] != last:
            raise ValueError(f"{what}: expected shape (N,H,W,{last}), got {tuple(t.shape)}")
        return t.contiguous()

    def encode(self, x, prequant: bool = False, out=None):
        """(N,H,W,3) u8 -> (N,ceil(H/8),ceil(W/8),96) u8 [, fp32 clipped pre-quant latent]."""
        torch = _torch()
        x = self._check_dev(x, 4, 3, "encode")
        n, h, w, _ = x.shape
        h8, w8 = _lib.latent_shape(h, w)
        z = out if out is not None else torch.empty((n, h8, w8, 96), dtype=torch.uint8, device=x.device)
        f = torch.empty((n, h8, w8, 96), dtype=torch.float32, device=x.device) if prequant else None
        rc = self._L.nic_encode(self._h, x.data_ptr(), n, h, w, z.data_ptr(), f.data_ptr() if f is not None else None,
                                _stream_ptr(torch, self.device))
        _lib.check(rc, "nic_encode")
        return (z, f) if prequant else z

    def encode_entropy(self, x, counts: bool = False, out=None):
        """encode(x) and entropy(latent) in one pass (nic_encode_entropy: the codes are counted
        in conv8's epilogue): (latent, (3N,) fp32 bits/symbol [, (3N,256) int32 counts])."""
        torch = _torch()
        x = self._check_dev(x, 4, 3, "encode_entropy")
        n, h, w, _ = x.shape
        h8, w8 = _lib.latent_shape(h, w)
        z = out if out is not None else torch.empty((n, h8, w8, 96), dtype=torch.uint8, device=x.device)
        bits = torch.empty((3 * n,), dtype=torch.float32, device=x.device)
        cnt = torch.empty((3 * n, 256), dtype=torch.int32, device=x.device) if counts else None
        rc = self._L.nic_encode_entropy(self._h, x.data_ptr(), n, h, w, z.data_ptr(),
                                        cnt.data_ptr() if cnt is not None else None, bits.data_ptr(),
                                        _stream_ptr(torch, self.device))
        _lib.check(rc, "nic_encode_entropy")
        return (z, bits, cnt) if counts else (z, bits)

    def encode_entropy_folds(self, n: int, h: int, w: int) -> bool:
        """True when encode_entropy on (n, h, w) images counts the codes inside conv8 (the fold),
        False when it runs encode + entropy (nic_encode_entropy_fold)."""
        import ctypes
        f = ctypes.c_int()
        _lib.check(self._L.nic_encode_entropy_fold(self._h, n, h, w, ctypes.byref(f)), "nic_encode_entropy_fold")
        return bool(f.value)

    def decode(self, z, rgb_f32: bool = False, out=None):
        """(N,h,w,96) u8 -> (N,8h,8w,3) u8 [, fp32 clipped RGB before quantisation]."""
        torch = _torch()
        z = self._check_dev(z, 4, 96, "decode")
        n, h8, w8, _ = z.shape
        x = out if out is not None else torch.empty((n, 8 * h8, 8 * w8, 3), dtype=torch.uint8, device=z.device)
        f = torch.empty((n, 8 * h8, 8 * w8, 3), dtype=torch.float32, device=z.device) if rgb_f32 else None
        rc = self._L.nic_decode(self._h, z.data_ptr(), n, h8, w8, x.data_ptr(), f.data_ptr() if f is not None else None,
                                _stream_ptr(torch, self.device))
        _lib.check(rc, "nic_decode")
        return (x, f) if rgb_f32 else x

    # -- host entry points (NumPy u8 arrays; nic_encode_host / nic_decode_host) ----------
    def _host_out(self, shape):
        """A u8 result array in page-locked memory (torch's caching host allocator): the D2H
        DMA lands in it directly, and a Decoder handed an Encoder result DMA's it directly."""
        torch = _torch()
        n = int(np.prod(shape))
        return torch.empty(max(n, 1), dtype=torch.uint8, pin_memory=True).numpy()[:n].reshape(shape)

    def encode_host(self, x: np.ndarray, chunks: int = 3) -> np.ndarray:
        """(N,H,W,3) u8 host array -> (N,ceil(H/8),ceil(W/8),96) u8 host array (synchronous)."""
        torch = _torch()
        x = np.ascontiguousarray(x, dtype=np.uint8)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError(f"encode_host: expected shape (N,H,W,3), got {x.shape}")
        n, h, w, _ = x.shape
        h8, w8 = _lib.latent_shape(h, w) if h > 0 and w > 0 else (0, 0)
        z = self._host_out((n, h8, w8, 96))
        rc = self._L.nic_encode_host(self._h, x.ctypes.data, n, h, w, z.ctypes.data, int(chunks),
                                     _stream_ptr(torch, self.device))
        _lib.check(rc, "nic_encode_host")
        return z

    def decode_host(self, z: np.ndarray, chunks: int = 3) -> np.ndarray:
        """(N,h,w,96) u8 host array -> (N,8h,8w,3) u8 host array (synchronous)."""
        torch = _torch()
        z = np.ascontiguousarray(z, dtype=np.uint8)
        if z.ndim != 4 or z.shape[3] != 96:
            raise ValueError(f"decode_host: expected shape (N,h,w,96), got {z.shape}")
        n, h8, w8, _ = z.shape
        x = self._host_out((n, 8 * h8, 8 * w8, 3))
        rc = self._L.nic_decode_host(self._h, z.ctypes.data, n, h8, w8, x.ctypes.data, int(chunks),
                                     _stream_ptr(torch, self.device))
        _lib.check(rc, "nic_decode_host")
        return x

    def entropy(self, z, counts: bool = False):
        """Histogram entropy per latent plane: (3N,) fp32 bits/symbol [, (3N,256) int32 counts]."""
        torch = _torch()
        z = self._check_dev(z, 4, 96, "entropy")
        n, h8, w8, _ = z.shape
        bits = torch.empty((3 * n,), dtype=torch.float32, device=z.device)
        cnt = torch.empty((3 * n, 256), dtype=torch.int32, device=z.device) if counts else None
        rc = self._L.nic_entropy_hist(self._h, z.data_ptr(), n, h8, w8, cnt.data_ptr() if cnt is not None else None,
                                      bits.data_ptr(), _stream_ptr(torch, self.device))
        _lib.check(rc, "nic_entropy_hist")
        return (bits, cnt) if counts else bits

    def ms_ssim(self, a, b, per_scale: bool = False):
        """tf.image.ssim_multiscale(a, b, max_val=255) per image (calc_ssim.py:13): (N,) fp32
        [, (N,3,5,2) mean SSIM / mean cs per channel and scale]."""
        torch = _torch()
        a = self._check_dev(a, 4, 3, "ms_ssim")
        b = self._check_dev(b, 4, 3, "ms_ssim")
        if a.shape != b.shape:
            raise ValueError(f"ms_ssim: shapes differ {tuple(a.shape)} vs {tuple(b.shape)}")
        n, h, w, _ = a.shape
        out = torch.empty((n,), dtype=torch.float32, device=a.device)
        ps = torch.empty((n, 3, 5, 2), dtype=torch.float32, device=a.device) if per_scale else None
        rc = self._L.nic_ms_ssim(self._h, a.data_ptr(), b.data_ptr(), n, h, w, out.data_ptr(),
                                 ps.data_ptr() if ps is not None else None, _stream_ptr(torch, self.device))
        _lib.check(rc, "nic_ms_ssim")
        return (out, ps) if per_scale else out

    def sq_err(self, a, b):
        """Exact per-image sum of squared differences of two u8 tensors (N,...): (N,) int64."""
        torch = _torch()
        for t in (a, b):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device.type != "cuda":
                raise TypeError("sq_err: expected cuda torch.uint8 tensors")
            if t.device.index != self.device:  # nic_sq_err launches on this codec's stream
                raise ValueError(f"sq_err: tensor on cuda:{t.device.index}, codec on cuda:{self.device}")
        if a.shape != b.shape or a.ndim < 1:
            raise ValueError(f"sq_err: shapes differ {tuple(a.shape)} vs {tuple(b.shape)}")
        a, b = a.contiguous(), b.contiguous()
        n = a.shape[0]
        out = torch.empty((n,), dtype=torch.int64, device=a.device)
        per = a.numel() // n if n else 0
        _lib.check(self._L.nic_sq_err(a.data_ptr(), b.data_ptr(), n, per, out.data_ptr(),
                                      _stream_ptr(torch, self.device)), "nic_sq_err")
        return out

    def psnr(self, a, b, max_val: float = 255.0, per_image: bool = False):
        """PSNR in dB over the whole batch (as the oracle's psnr) or per image, from the exact
        device sum of squared errors.  Reads the sums back to the host (synchronises)."""
        import math

        sse = self.sq_err(a, b).cpu().numpy().astype(np.float64)
        n = a.shape[0]
        per = a.numel() // n if n else 0

        def db(s, count):
            return float("inf") if s == 0 else 10.0 * math.log10(max_val ** 2 * count / s)

        if per_image:
            return np.array([db(s, per) for s in sse])
        return db(float(sse.sum()), per * n)

    # -- .nic container: device rANS coder (nic_rans_*) -----------------------------------
    def rans_reserve(self, n: int, h8: int, w8: int, seg_pixels: int = 32) -> None:
        """Grow the workspace so rans_encode / rans_decode of (n, h8, w8) latents allocate nothing."""
        _lib.check(self._L.nic_rans_reserve(self._h, n, h8, w8, seg_pixels), "nic_rans_reserve")

    # One body per call for the three container versions: ver picks nic_rans_*, nic_rans2_* or
    # nic_rans3_*, and the public method's name in the error texts.
    _RANS = {1: "rans", 2: "rans2", 3: "rans3"}

    def _rans_encode(self, ver: int, z, seg_pixels, size=None):
        torch = _torch()
        name = self._RANS[ver] + "_encode"
        z = self._check_dev(z, 4, 96, name)
        n, h8, w8, _ = z.shape
        if z.data_ptr() % 16:  # a view at an odd offset: the kernels read 16-byte words
            z = z.clone()
        hw = ()  # version 1 does not record the image size
        if ver != 1:
            hw = (8 * h8, 8 * w8) if size is None else (int(size[0]), int(size[1]))
        stride = ctypes.c_int64()
        bound = f"nic_{self._RANS[ver]}_bound"
        _lib.check(getattr(self._L, bound)(h8, w8, int(seg_pixels), ctypes.byref(stride)), bound)
        buf = torch.empty((n, stride.value), dtype=torch.uint8, device=z.device)
        sizes = torch.zeros((n,), dtype=torch.int64, device=z.device)
        _lib.check(getattr(self._L, "nic_" + name)(self._h, z.data_ptr(), n, h8, w8, *hw, int(seg_pixels), buf.data_ptr(),
                                                   stride.value, sizes.data_ptr(), _stream_ptr(torch, self.device)),
                   "nic_" + name)
        return buf, sizes

    def _rans_decode_status(self, ver: int, buf, sizes, h8: int, w8: int, out=None, window=None):
        """window None: the whole (N,h8,w8,96) latents; else (r0, c0, rows, cols): that window of them."""
        torch = _torch()
        name = self._RANS[ver] + ("_decode" if window is None else "_decode_window")
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.device.type != "cuda" or buf.ndim != 2:
            raise TypeError(f"{name}: expected an (N, stride) cuda torch.uint8 tensor of files")
        if not isinstance(sizes, torch.Tensor) or sizes.dtype != torch.int64 or sizes.shape != (buf.shape[0],):
            raise TypeError(f"{name}: expected an (N,) torch.int64 tensor of sizes")
        if buf.device.index != self.device or sizes.device != buf.device:
            raise ValueError(f"{name}: tensors must be on cuda:{self.device}")
        buf, sizes = buf.contiguous(), sizes.contiguous()
        n, stride = buf.shape
        if window is None:
            win, shape, text = (), (n, h8, w8, 96), "(N,h8,w8,96)"
        else:
            win = tuple(int(v) for v in window)
            shape, text = (n, win[2], win[3], 96), "(N,rows,cols,96)"
        if out is None:
            if window is not None:  # a bad window is nic_rans*_decode_window's to report
                shape = (n, max(win[2], 0), max(win[3], 0), 96)
            out = torch.empty(shape, dtype=torch.uint8, device=buf.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != buf.device or not out.is_contiguous():
            raise TypeError(f"{name}: out must be a contiguous {text} torch.uint8 tensor on the codec's device")
        status = torch.zeros((n,), dtype=torch.int32, device=buf.device)
        _lib.check(getattr(self._L, "nic_" + name)(self._h, buf.data_ptr(), stride, sizes.data_ptr(), n, int(h8), int(w8), *win,
                                                   out.data_ptr(), status.data_ptr(), _stream_ptr(torch, self.device)),
                   "nic_" + name)
        return out, status

    def _rans_decode(self, ver: int, buf, sizes, h8: int, w8: int, window=None):
        z, status = self._rans_decode_status(ver, buf, sizes, h8, w8, window=window)
        self._rans_raise(self._RANS[ver] + ("_decode" if window is None else "_decode_window"), ver, buf, status)
        return z

    def _rans_raise(self, name: str, ver: int, buf, status) -> None:
        """Reads the statuses back (synchronises); ValueError naming the first image with one set."""
        st = status.cpu().numpy()
        bad = np.nonzero(st)[0]
        if bad.size:
            i = int(bad[0])
            if ver != 1 and st[i] & 8:
                pid = int.from_bytes(bytes(buf[i, 24:28].cpu().numpy().tolist()), "little")
                mine = self.prior if ver == 2 else self.context_prior
                raise ValueError(f"{name}: image {i} was written under prior {pid:08x}, the codec's prior is "
                                 f"{mine.id:08x} (status {int(st[i])}; refused images: {bad.tolist()})")
            raise ValueError(f"{name}: image {i} is corrupt (status {int(st[i])}; corrupt images: {bad.tolist()})")

    def rans_encode(self, z, seg_pixels: int = 32):
        """(N,h,w,96) u8 latent -> (buf (N, stride) u8, sizes (N,) int64), device tensors: image
        i's complete .nic file is buf[i, :sizes[i]] (nic_rans_encode; no host synchronisation)."""
        return self._rans_encode(1, z, seg_pixels)

    def rans_decode_status(self, buf, sizes, h8: int, w8: int, out=None):
        """rans_decode without the check: (latent, status (N,) int32 device tensor; nic.h).
        out: the (N,h8,w8,96) u8 tensor to decode into (default: a new one)."""
        return self._rans_decode_status(1, buf, sizes, h8, w8, out)

    def rans_decode(self, buf, sizes, h8: int, w8: int):
        """.nic files buf[i, :sizes[i]] (device tensors, as rans_encode returns) of (h8, w8)
        latents -> (N,h8,w8,96) u8.  Reads the statuses back (synchronises) and raises ValueError
        naming the first image whose file did not decode cleanly."""
        return self._rans_decode(1, buf, sizes, h8, w8)


    # -- .nic version 2: the codec-level prior (nic_rans_prior_*, nic_rans2_*) -----------------
    #: the Prior set by set_prior (None: version-1 files only)
    prior = None

    def set_prior(self, prior) -> None:
        """The prior (prior.Prior) of rans2_encode / rans2_decode, or None to clear it
        (nic_rans_prior_set: synchronous)."""
        if prior is None:
            _lib.check(self._L.nic_rans_prior_set(self._h, None, None), "nic_rans_prior_set")
            self.prior = None
            return
        pid = ctypes.c_uint32()
        _lib.check(self._L.nic_rans_prior_set(self._h, prior.freqs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pid)),
                   "nic_rans_prior_set")
        assert pid.value == prior.id
        self.prior = prior

    def prior_count(self, z, counts) -> None:
        """Adds the per-channel symbol counts of the latents z (N,h,w,96) into counts, a (96, 256)
        int64 device tensor read as uint64 (nic_rans_prior_count; no host synchronisation)."""
        torch = _torch()
        z = self._check_dev(z, 4, 96, "prior_count")
        if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.shape != (96, 256)
                or counts.device != z.device or not counts.is_contiguous()):
            raise TypeError("prior_count: counts must be a contiguous (96, 256) torch.int64 tensor on the codec's device")
        n, h8, w8, _ = z.shape
        if z.data_ptr() % 16:
            z = z.clone()
        _lib.check(self._L.nic_rans_prior_count(self._h, z.data_ptr(), n, h8, w8, counts.data_ptr(),
                                                _stream_ptr(torch, self.device)), "nic_rans_prior_count")

    def prior_build(self, counts):
        """(96, 256) int64 device counts -> (96, 256) freqs as an int32 device tensor
        (nic_rans_prior_build; no host synchronisation)."""
        torch = _torch()
        if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.shape != (96, 256)
                or counts.device.type != "cuda" or counts.device.index != self.device):
            raise TypeError("prior_build: counts must be a (96, 256) torch.int64 tensor on the codec's device")
        counts = counts.contiguous()
        freqs = torch.empty((96, 256), dtype=torch.int16, device=counts.device)  # u16 bits, all <= 4096
        _lib.check(self._L.nic_rans_prior_build(self._h, counts.data_ptr(), freqs.data_ptr(),
                                                _stream_ptr(torch, self.device)), "nic_rans_prior_build")
        return freqs.to(torch.int32)

    def rans2_reserve(self, n: int, h8: int, w8: int, seg_pixels: int = 32) -> None:
        """Grow the workspace so rans2_encode / rans2_decode of (n, h8, w8) latents allocate nothing."""
        _lib.check(self._L.nic_rans2_reserve(self._h, n, h8, w8, seg_pixels), "nic_rans2_reserve")

    def rans2_encode(self, z, seg_pixels: int = 32, size=None):
        """rans_encode with the codec's prior: version-2 files, which store a table only for the
        channels where it pays and record the images' own size=(H, W) (default 8 h x 8 w).
        NicError(NIC_ENOPRIOR) without a prior."""
        return self._rans_encode(2, z, seg_pixels, size)

    def rans2_decode_status(self, buf, sizes, h8: int, w8: int, out=None):
        """rans2_decode without the check: (latent, status (N,) int32 device tensor; nic.h).
        out: the (N,h8,w8,96) u8 tensor to decode into (default: a new one)."""
        return self._rans_decode_status(2, buf, sizes, h8, w8, out)

    def rans2_decode(self, buf, sizes, h8: int, w8: int):
        """Version-2 .nic files buf[i, :sizes[i]] of (h8, w8) latents -> (N,h8,w8,96) u8.  Reads the
        statuses back (synchronises) and raises ValueError naming the first image whose file did
        not decode cleanly; a file written under another prior is reported with both ids."""
        return self._rans_decode(2, buf, sizes, h8, w8)


    # -- .nic version 3: the context prior (nic_rans_cprior_*, nic_rans3_*) ---------------------
    #: the ContextPrior set by set_context_prior (None: no version-3 files)
    context_prior = None

    def set_context_prior(self, cprior) -> None:
        """The context prior (prior.ContextPrior) of rans3_encode / rans3_decode, or None to clear
        it (nic_rans_cprior_set: synchronous).  Independent of set_prior."""
        if cprior is None:
            _lib.check(self._L.nic_rans_cprior_set(self._h, None, None, None), "nic_rans_cprior_set")
            self.context_prior = None
            return
        pid = ctypes.c_uint32()
        _lib.check(self._L.nic_rans_cprior_set(self._h, cprior.anchors.ctypes.data_as(ctypes.c_void_p),
                                               cprior.freqs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pid)),
                   "nic_rans_cprior_set")
        assert pid.value == cprior.id
        self.context_prior = cprior

    def cprior_count(self, z, anchors, counts, seg_pixels: int = 32) -> None:
        """Adds the context counts of the latents z (N,h,w,96), cut into segments of seg_pixels,
        under anchors ((96,) u8 device tensor) into counts, a (96, 3, 256) int64 device tensor read
        as uint64 (nic_rans_cprior_count; no host synchronisation)."""
        torch = _torch()
        z = self._check_dev(z, 4, 96, "cprior_count")
        if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.shape != (96, 3, 256)
                or counts.device != z.device or not counts.is_contiguous()):
            raise TypeError("cprior_count: counts must be a contiguous (96, 3, 256) torch.int64 tensor on the codec's device")
        if (not isinstance(anchors, torch.Tensor) or anchors.dtype != torch.uint8 or anchors.shape != (96,)
                or anchors.device != z.device or not anchors.is_contiguous()):
            raise TypeError("cprior_count: anchors must be a contiguous (96,) torch.uint8 tensor on the codec's device")
        n, h8, w8, _ = z.shape
        if z.data_ptr() % 16:
            z = z.clone()
        _lib.check(self._L.nic_rans_cprior_count(self._h, z.data_ptr(), n, h8, w8, int(seg_pixels), anchors.data_ptr(),
                                                 counts.data_ptr(), _stream_ptr(torch, self.device)), "nic_rans_cprior_count")

    def cprior_build(self, counts):
        """(96, 3, 256) int64 device counts -> (96, 3, 256) freqs as an int32 device tensor
        (nic_rans_cprior_build; no host synchronisation)."""
        torch = _torch()
        if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.shape != (96, 3, 256)
                or counts.device.type != "cuda" or counts.device.index != self.device):
            raise TypeError("cprior_build: counts must be a (96, 3, 256) torch.int64 tensor on the codec's device")
        counts = counts.contiguous()
        freqs = torch.empty((96, 3, 256), dtype=torch.int16, device=counts.device)  # u16 bits, all <= 4096
        _lib.check(self._L.nic_rans_cprior_build(self._h, counts.data_ptr(), freqs.data_ptr(),
                                                 _stream_ptr(torch, self.device)), "nic_rans_cprior_build")
        return freqs.to(torch.int32)

    def rans3_reserve(self, n: int, h8: int, w8: int, seg_pixels: int = 32) -> None:
        """Grow the workspace so rans3_encode / rans3_decode of (n, h8, w8) latents allocate nothing."""
        _lib.check(self._L.nic_rans3_reserve(self._h, n, h8, w8, seg_pixels), "nic_rans3_reserve")

    def rans3_encode(self, z, seg_pixels: int = 32, size=None):
        """rans2_encode with the codec's context prior: version-3 files, whose symbols are coded
        under the row their left neighbour selects.  NicError(NIC_ENOPRIOR) without a context prior."""
        return self._rans_encode(3, z, seg_pixels, size)

    def rans3_decode_status(self, buf, sizes, h8: int, w8: int, out=None):
        """rans3_decode without the check: (latent, status (N,) int32 device tensor; nic.h).
        out: the (N,h8,w8,96) u8 tensor to decode into (default: a new one)."""
        return self._rans_decode_status(3, buf, sizes, h8, w8, out)

    def rans3_decode(self, buf, sizes, h8: int, w8: int):
        """Version-3 .nic files buf[i, :sizes[i]] of (h8, w8) latents -> (N,h8,w8,96) u8.  Reads the
        statuses back (synchronises) and raises ValueError naming the first image whose file did
        not decode cleanly; a file written under another context prior is reported with both ids."""
        return self._rans_decode(3, buf, sizes, h8, w8)


    # -- rate-distortion optimised quantisation against the codec's prior (nic_rdoq) -------------
    #: the largest lambda of rdoq (lam_fix = round(lam * 65536) stays inside nic_rdoq's range)
    RDOQ_LAM_MAX = 16.0

    def rdoq(self, z, f, lam: float, seg_pixels: int = 32, prior=None, out=None):
        """Codes z (N,h,w,96) u8 and their pre-quant values f (N,h,w,96) fp32, as encode(x,
        prequant=True) returns them -> the codes that cost least in distortion + lam x bits under the
        codec's prior: every code stays or moves one step towards its pre-quant value (nic_rdoq; no
        host synchronisation).  prior: "static" (set_prior; every code on its own), "context"
        (set_context_prior; every (segment, channel) chain of seg_pixels in 1..64 pixels as a whole),
        or None: whichever is set, the context prior first, as nic_files prefers.  lam in [0, 16]; 0
        returns z's codes.  out: the (N,h,w,96) u8 tensor to write (not z; default: a new one).
        NicError(NIC_ENOPRIOR) when that prior is not set."""
        torch = _torch()
        z = self._check_dev(z, 4, 96, "rdoq")
        if (not isinstance(f, torch.Tensor) or f.dtype != torch.float32 or f.device != z.device
                or tuple(f.shape) != tuple(z.shape)):
            raise TypeError("rdoq: f must be a torch.float32 tensor of z's shape on the codec's device")
        if prior not in (None, "static", "context"):
            raise ValueError(f'rdoq: prior must be "static", "context" or None, got {prior!r}')
        lam = float(lam)
        if not 0.0 <= lam <= self.RDOQ_LAM_MAX:  # also refuses NaN
            raise ValueError(f"rdoq: lam {lam} not in [0, {self.RDOQ_LAM_MAX:g}]")
        if prior is None:
            prior = "static" if self.context_prior is None and self.prior is not None else "context"
        f = f.contiguous()
        if z.data_ptr() % 16:
            z = z.clone()
        if f.data_ptr() % 16:
            f = f.clone()
        if out is None:
            out = torch.empty_like(z)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(z.shape)
              or out.device != z.device or not out.is_contiguous()):
            raise TypeError("rdoq: out must be a contiguous (N,h,w,96) torch.uint8 tensor on the codec's device")
        n, h8, w8, _ = z.shape
        _lib.check(self._L.nic_rdoq(self._h, z.data_ptr(), f.data_ptr(), n, h8, w8, int(seg_pixels), int(round(lam * 65536)),
                                    3 if prior == "context" else 1, out.data_ptr(), _stream_ptr(torch, self.device)),
                   "nic_rdoq")
        return out


    # -- region decode: a latent window out of .nic files (nic_region_plan, nic_rans*_decode_window) --
    @staticmethod
    def region_plan(H: int, W: int, box):
        """The latent window and the cut for box = (y, x, h, w) of an H x W image (nic_region_plan;
        host only): ((r0, c0, rows, cols), (off_y, off_x)) -- the window holds every latent pixel
        the box's pixels depend on, and the box is [off_y : off_y + h, off_x : off_x + w] of the
        window's reconstruction.  ValueError for a box that does not lie inside the image."""
        y, x, bh, bw = (int(v) for v in box)
        win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
        _lib.check(_lib.lib().nic_region_plan(int(H), int(W), y, x, bh, bw, win, off), "nic_region_plan")
        return tuple(win), tuple(off)

    def rans_decode_window_status(self, buf, sizes, h8: int, w8: int, window, out=None):
        """rans_decode_window without the check: (window latent, status (N,) int32 device tensor).
        out: the (N,rows,cols,96) u8 tensor to decode into (default: a new one)."""
        return self._rans_decode_status(1, buf, sizes, h8, w8, out, window)

    def rans_decode_window(self, buf, sizes, h8: int, w8: int, window):
        """The window = (r0, c0, rows, cols) of the (h8, w8) latents of version-1 .nic files
        buf[i, :sizes[i]] -> (N,rows,cols,96) u8, the slice [:, r0:r0+rows, c0:c0+cols] of rans_decode's
        result; only the segments that hold a pixel of the window are decoded
        (nic_rans_decode_window).  Reads the statuses back (synchronises) and raises ValueError naming
        the first image that did not decode cleanly; damage outside those segments is not seen."""
        return self._rans_decode(1, buf, sizes, h8, w8, window)

    def rans2_decode_window_status(self, buf, sizes, h8: int, w8: int, window, out=None):
        """rans2_decode_window without the check (as rans_decode_window_status)."""
        return self._rans_decode_status(2, buf, sizes, h8, w8, out, window)

    def rans2_decode_window(self, buf, sizes, h8: int, w8: int, window):
        """rans_decode_window for version-2 files, under the codec's prior (NicError(NIC_ENOPRIOR)
        without one; a file written under another prior is reported with both ids)."""
        return self._rans_decode(2, buf, sizes, h8, w8, window)

    def rans3_decode_window_status(self, buf, sizes, h8: int, w8: int, window, out=None):
        """rans3_decode_window without the check (as rans_decode_window_status)."""
        return self._rans_decode_status(3, buf, sizes, h8, w8, out, window)

    def rans3_decode_window(self, buf, sizes, h8: int, w8: int, window):
        """rans_decode_window for version-3 files, under the codec's context prior
        (NicError(NIC_ENOPRIOR) without one)."""
        return self._rans_decode(3, buf, sizes, h8, w8, window)

    # -- batched region decode: a window per file, one shape per call (nic_region_plan_fixed,
    # nic_rans*_decode_windows, nic_cut_boxes) --
    @staticmethod
    def region_plan_fixed(H: int, W: int, box):
        """region_plan with a window whose shape depends on the box's size alone, unless the latent is
        smaller (nic_region_plan_fixed; host only): ((r0, c0, rows, cols), (off_y, off_x)) with rows =
        min(h8, (h + 6) // 8 + 1 + 2 NIC_DECODE_HALO), likewise cols, so boxes of one size out of images
        of any sizes give windows of one shape.  The window holds region_plan's; the cut is as exact."""
        y, x, bh, bw = (int(v) for v in box)
        win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
        _lib.check(_lib.lib().nic_region_plan_fixed(int(H), int(W), y, x, bh, bw, win, off), "nic_region_plan_fixed")
        return tuple(win), tuple(off)

    def _device_table(self, table, cols: int, name: str, what: str):
        """An (N, cols) int32 table for the device: a contiguous tensor there, or host values uploaded.
        Returns (device tensor, host array or None)."""
        torch = _torch()
        if isinstance(table, torch.Tensor) and table.device.type == "cuda":
            if table.dtype != torch.int32 or table.ndim != 2 or table.shape[1] != cols or table.device.index != self.device:
                raise TypeError(f"{name}: {what} must be an (N,{cols}) torch.int32 tensor on cuda:{self.device}")
            return table.contiguous(), None
        host = np.ascontiguousarray(np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table, dtype=np.int64))
        if host.size == 0:
            host = host.reshape(0, cols)
        if host.ndim != 2 or host.shape[1] != cols or (host.size and np.abs(host).max() >= 2 ** 31):
            raise ValueError(f"{name}: {what} must be N rows of {cols} 32-bit integers")
        return torch.from_numpy(host.astype(np.int32)).to(f"cuda:{self.device}"), host

    def _rans_decode_windows_status(self, ver: int, buf, sizes, table, shape, max_pixels=None, out=None):
        torch = _torch()
        name = self._RANS[ver] + "_decode_windows"
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.device.type != "cuda" or buf.ndim != 2:
            raise TypeError(f"{name}: expected an (N, stride) cuda torch.uint8 tensor of files")
        if not isinstance(sizes, torch.Tensor) or sizes.dtype != torch.int64 or sizes.shape != (buf.shape[0],):
            raise TypeError(f"{name}: expected an (N,) torch.int64 tensor of sizes")
        if buf.device.index != self.device or sizes.device != buf.device:
            raise ValueError(f"{name}: tensors must be on cuda:{self.device}")
        buf, sizes = buf.contiguous(), sizes.contiguous()
        n, stride = buf.shape
        rows, cols = (int(v) for v in shape)
        tab, host = self._device_table(table, 4, name, "table")
        if tab.shape[0] != n:
            raise ValueError(f"{name}: {tab.shape[0]} table rows for {n} files")
        if max_pixels is None:
            if host is None:
                raise ValueError(f"{name}: a table on the device needs max_pixels, the bound on h8 * w8 of its rows")
            # the largest latent a row names; rows that name none, or too large a one, are the device's to refuse
            pixels = [a * b for a, b in host[:, :2].tolist() if a > 0 and b > 0 and a * b <= 1 << 23]
            max_pixels = min(max(pixels + [rows * cols, 1]), 1 << 23)
        if out is None:
            out = torch.empty((n, max(rows, 0), max(cols, 0), 96), dtype=torch.uint8, device=buf.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (n, rows, cols, 96) or out.device != buf.device or not out.is_contiguous():
            raise TypeError(f"{name}: out must be a contiguous (N,rows,cols,96) torch.uint8 tensor on the codec's device")
        status = torch.zeros((n,), dtype=torch.int32, device=buf.device)
        _lib.check(getattr(self._L, "nic_" + name)(self._h, buf.data_ptr(), stride, sizes.data_ptr(), n, tab.data_ptr(),
                                                   int(max_pixels), rows, cols, out.data_ptr(), status.data_ptr(),
                                                   _stream_ptr(torch, self.device)), "nic_" + name)
        return out, status

    def _rans_decode_windows(self, ver: int, buf, sizes, table, shape, max_pixels=None):
        z, status = self._rans_decode_windows_status(ver, buf, sizes, table, shape, max_pixels)
        self._rans_raise(self._RANS[ver] + "_decode_windows", ver, buf, status)
        return z

    def rans_decode_windows_status(self, buf, sizes, table, shape, max_pixels=None, out=None):
        """rans_decode_windows without the check: (window latents, status (N,) int32 device tensor).
        out: the (N,rows,cols,96) u8 tensor to decode into (default: a new one)."""
        return self._rans_decode_windows_status(1, buf, sizes, table, shape, max_pixels, out)

    def rans_decode_windows(self, buf, sizes, table, shape, max_pixels=None):
        """A window of shape = (rows, cols) out of each of the version-1 .nic files buf[i, :sizes[i]],
        which may hold latents of different sizes: row i of table is file i's (h8, w8, r0, c0), and the
        result (N,rows,cols,96) u8 holds [r0:r0+rows, c0:c0+cols] of file i's latent
        (nic_rans_decode_windows).  table: N rows of host integers, uploaded here, or an (N,4) int32
        tensor on the device, which then needs max_pixels, a bound on h8 * w8 of every row (it sizes
        the workspace; from host rows it is computed).  A row that does not match its file's header,
        exceeds the bound, or whose window does not fit its latent is refused on the device with the
        header bit (status 2).  Reads the statuses back (synchronises) and raises ValueError naming the
        first image that was refused or did not decode cleanly."""
        return self._rans_decode_windows(1, buf, sizes, table, shape, max_pixels)

    def rans2_decode_windows_status(self, buf, sizes, table, shape, max_pixels=None, out=None):
        """rans2_decode_windows without the check (as rans_decode_windows_status)."""
        return self._rans_decode_windows_status(2, buf, sizes, table, shape, max_pixels, out)

    def rans2_decode_windows(self, buf, sizes, table, shape, max_pixels=None):
        """rans_decode_windows for version-2 files, under the codec's prior."""
        return self._rans_decode_windows(2, buf, sizes, table, shape, max_pixels)

    def rans3_decode_windows_status(self, buf, sizes, table, shape, max_pixels=None, out=None):
        """rans3_decode_windows without the check (as rans_decode_windows_status)."""
        return self._rans_decode_windows_status(3, buf, sizes, table, shape, max_pixels, out)

    def rans3_decode_windows(self, buf, sizes, table, shape, max_pixels=None):
        """rans_decode_windows for version-3 files, under the codec's context prior."""
        return self._rans_decode_windows(3, buf, sizes, table, shape, max_pixels)

    def cut_boxes(self, x, offsets, h: int, w: int, out=None):
        """The h x w box at offsets[i] = (oy, ox) of image i of x (N,Hs,Ws,3) u8 -> (N,h,w,3) u8, one
        launch on the current stream (nic_cut_boxes).  offsets: N pairs of host integers, checked here
        against the images (ValueError naming the row) and uploaded, or an (N,2) int32 tensor on the
        device, which is not read back: there a source pixel outside its image reads as 0."""
        torch = _torch()
        x = self._check_dev(x, 4, 3, "cut_boxes")
        n, Hs, Ws, _ = x.shape
        h, w = int(h), int(w)
        off, host = self._device_table(offsets, 2, "cut_boxes", "offsets")
        if off.shape[0] != n:
            raise ValueError(f"cut_boxes: {off.shape[0]} offsets for {n} images")
        if host is not None:
            for i, (oy, ox) in enumerate(host.tolist()):
                if oy < 0 or ox < 0 or oy + h > Hs or ox + w > Ws:
                    raise ValueError(f"cut_boxes: image {i}: a {h} x {w} box at ({oy}, {ox}) does not lie inside the "
                                     f"{Hs} x {Ws} images")
        if out is None:
            out = torch.empty((n, max(h, 0), max(w, 0), 3), dtype=torch.uint8, device=x.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or out.device != x.device or not out.is_contiguous():
            raise TypeError("cut_boxes: out must be a contiguous (N,h,w,3) torch.uint8 tensor on the codec's device")
        _lib.check(self._L.nic_cut_boxes(self._h, x.data_ptr(), n, Hs, Ws, off.data_ptr(), h, w, out.data_ptr(),
                                         _stream_ptr(torch, self.device)), "nic_cut_boxes")
        return out

    # -- crops of mixed sizes, resized for training (nic_region_plan_window, nic_resample_boxes) --
    @staticmethod
    def region_plan_window(H: int, W: int, box, shape):
        """region_plan_fixed with the window's shape given (nic_region_plan_window; host only):
        ((r0, c0, rows, cols), (off_y, off_x)) with rows = min(h8, shape[0]), cols = min(w8, shape[1]).
        shape must be at least the fixed plan's (h + 6) // 8 + 1 + 2 NIC_DECODE_HALO per axis
        (ValueError), so boxes of different sizes can share the largest one's window shape; the cut
        is as exact as region_plan's."""
        y, x, bh, bw = (int(v) for v in box)
        rows, cols = (int(v) for v in shape)
        win, off = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
        _lib.check(_lib.lib().nic_region_plan_window(int(H), int(W), y, x, bh, bw, rows, cols, win, off),
                   "nic_region_plan_window")
        return tuple(win), tuple(off)

    @staticmethod
    def window_need(h: int, w: int):
        """The smallest window shape region_plan_window takes for an h x w box: the fixed plan's (R, C)."""
        return tuple((int(v) + 6) // 8 + 1 + 2 * _lib.DECODE_HALO for v in (h, w))

    _RESAMPLE_KINDS = {"float32": 0, "float16": 1, "uint8": 2}  # nic.h NIC_RESAMPLE_*

    def resample_boxes(self, x, table, size, dtype=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), n_out=None, out=None):
        """Row i of table = (oy, ox, bh, bw, flip, dst): the bh x bw box at (oy, ox) of image i of x
        (N,Hs,Ws,3) u8, resized to size = (oh, ow) as F.interpolate(mode="bilinear", antialias=True)
        does, mirrored left to right where flip is 1, becomes image dst of the result; one launch on
        the current stream (nic_resample_boxes).  dtype torch.float32 (the default) or torch.float16:
        (n_out, 3, oh, ow), (v / 255 - mean[c]) / std[c] as one fma with scale 1 / (255 std) and bias
        -mean / std, computed in float64 and rounded to fp32.  torch.uint8: (n_out, oh, ow, 3), rounded
        half to even; mean and std are not used.  n_out: the result's image count (default N; the
        images no row names keep what they held).  out: the tensor to fill (default: a new one, not
        initialised).  table: N rows of host integers, checked here against the images and n_out
        (ValueError naming the row) and uploaded, or an (N,6) int32 tensor on the device, which is not
        read back: there a row that does not fit is skipped by the kernel."""
        torch = _torch()
        x = self._check_dev(x, 4, 3, "resample_boxes")
        n, Hs, Ws, _ = x.shape
        dtype = torch.float32 if dtype is None else dtype
        kind = self._RESAMPLE_KINDS.get(str(dtype).replace("torch.", ""))
        if kind is None:
            raise ValueError(f"resample_boxes: dtype {dtype} is not torch.float32, torch.float16 or torch.uint8")
        try:
            oh, ow = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"resample_boxes: size must be (oh, ow), got {size!r}") from None
        mean64, std64 = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
        if mean64.shape != (3,) or std64.shape != (3,) or not np.all(np.isfinite(mean64)) or not np.all(np.isfinite(std64)) \
                or np.any(std64 == 0):
            raise ValueError(f"resample_boxes: mean and std must be 3 finite numbers each, std not 0; got {mean!r}, {std!r}")
        scale = (1.0 / (255.0 * std64)).astype(np.float32)
        bias = (-mean64 / std64).astype(np.float32)
        tab, host = self._device_table(table, 6, "resample_boxes", "table")
        if tab.shape[0] != n:
            raise ValueError(f"resample_boxes: {tab.shape[0]} table rows for {n} images")
        if n_out is None:
            n_out = out.shape[0] if isinstance(out, torch.Tensor) and out.ndim == 4 else n
        n_out = int(n_out)
        if host is not None:
            for i, (oy, ox, bh, bw, flip, dst) in enumerate(host.tolist()):
                if bh < 1 or bw < 1 or oy < 0 or ox < 0 or oy + bh > Hs or ox + bw > Ws:
                    raise ValueError(f"resample_boxes: row {i}: a {bh} x {bw} box at ({oy}, {ox}) does not lie inside the "
                                     f"{Hs} x {Ws} images")
                if flip not in (0, 1):
                    raise ValueError(f"resample_boxes: row {i}: flip {flip} is not 0 or 1")
                if dst < 0 or dst >= n_out:
                    raise ValueError(f"resample_boxes: row {i}: dst {dst} is not one of the {n_out} output images")
        shape = (n_out, max(oh, 0), max(ow, 0), 3) if kind == 2 else (n_out, 3, max(oh, 0), max(ow, 0))
        if out is None:
            out = torch.empty(tuple(max(v, 0) for v in shape), dtype=dtype, device=x.device)
        elif out.dtype != dtype or tuple(out.shape) != shape or out.device != x.device or not out.is_contiguous():
            raise TypeError(f"resample_boxes: out must be a contiguous {shape} {dtype} tensor on the codec's device")
        _lib.check(self._L.nic_resample_boxes(self._h, x.data_ptr(), n, Hs, Ws, tab.data_ptr(), oh, ow, n_out, kind,
                                              scale.ctypes.data, bias.ctypes.data, out.data_ptr(),
                                              _stream_ptr(torch, self.device)), "nic_resample_boxes")
        return out

    # -- images of mixed sizes, resized in one launch (nic_resample_ragged) ---------------------
    def _resample_args(self, who: str, size, dtype, mean, std):
        torch = _torch()
        dtype = torch.float32 if dtype is None else dtype
        kind = self._RESAMPLE_KINDS.get(str(dtype).replace("torch.", ""))
        if kind is None:
            raise ValueError(f"{who}: dtype {dtype} is not torch.float32, torch.float16 or torch.uint8")
        try:
            oh, ow = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: size must be (oh, ow), got {size!r}") from None
        mean64, std64 = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
        if mean64.shape != (3,) or std64.shape != (3,) or not np.all(np.isfinite(mean64)) or not np.all(np.isfinite(std64)) \
                or np.any(std64 == 0):
            raise ValueError(f"{who}: mean and std must be 3 finite numbers each, std not 0; got {mean!r}, {std!r}")
        return dtype, kind, oh, ow, (1.0 / (255.0 * std64)).astype(np.float32), (-mean64 / std64).astype(np.float32)

    def resample_pool(self, pool, table, size, dtype=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), n_out=None, out=None):
        """nic_resample_ragged as it is: pool a 1-D u8 tensor on this device, table an (N, 8) int64
        tensor there, row i = (offset, Hs, Ws, oy, ox, bh, bw, dst | flip << 32) (nic.h).  The table is
        not read back: a row that does not fit its image, the pool or the result is skipped by the
        kernel.  size, dtype, mean, std, n_out, out and the result as resample_boxes'."""
        torch = _torch()
        who = "resample_pool"
        if not isinstance(pool, torch.Tensor) or pool.dtype != torch.uint8 or pool.device.type != "cuda" or pool.ndim != 1 \
                or pool.device.index != self.device or not pool.is_contiguous():
            raise TypeError(f"{who}: pool must be a contiguous 1-D torch.uint8 tensor on cuda:{self.device}")
        if not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.ndim != 2 or table.shape[1] != 8 \
                or table.device != pool.device or not table.is_contiguous():
            raise TypeError(f"{who}: table must be a contiguous (N,8) torch.int64 tensor on cuda:{self.device}")
        dtype, kind, oh, ow, scale, bias = self._resample_args(who, size, dtype, mean, std)
        n = table.shape[0]
        if n_out is None:
            n_out = out.shape[0] if isinstance(out, torch.Tensor) and out.ndim == 4 else n
        n_out = int(n_out)
        shape = (n_out, max(oh, 0), max(ow, 0), 3) if kind == 2 else (n_out, 3, max(oh, 0), max(ow, 0))
        if out is None:
            out = torch.empty(tuple(max(v, 0) for v in shape), dtype=dtype, device=pool.device)
        elif out.dtype != dtype or tuple(out.shape) != shape or out.device != pool.device or not out.is_contiguous():
            raise TypeError(f"{who}: out must be a contiguous {shape} {dtype} tensor on the codec's device")
        _lib.check(self._L.nic_resample_ragged(self._h, pool.data_ptr(), pool.numel(), n, table.data_ptr(), oh, ow, n_out, kind,
                                               scale.ctypes.data, bias.ctypes.data, out.data_ptr(),
                                               _stream_ptr(torch, self.device)), "nic_resample_ragged")
        return out

    def upload_pool(self, images):
        """(H, W, 3) u8 images of any sizes (NumPy arrays or torch tensors, on the host or on this
        device) -> (pool, offsets, shapes): one 1-D u8 tensor on this device that holds them all at
        pool_layout's offsets.  The host's images are packed into one page-locked buffer and go up in
        one transfer on the current stream; the device's are copied into their places there.
        ValueError naming the image that is not (H, W, 3) u8 with H, W >= 1 and H W <= 2^29."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        items = []
        for i, a in enumerate(images):
            on_dev = isinstance(a, torch.Tensor) and a.device.type == "cuda"
            if on_dev and a.device.index != self.device:
                raise ValueError(f"resample_ragged: image {i}: tensor on cuda:{a.device.index}, codec on cuda:{self.device}")
            if not on_dev:
                a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            ok = a.ndim == 3 and a.shape[2] == 3 and a.shape[0] >= 1 and a.shape[1] >= 1 and a.shape[0] * a.shape[1] <= 1 << 29
            if not ok or a.dtype != (torch.uint8 if on_dev else np.uint8):
                raise ValueError(f"resample_ragged: image {i}: expected an (H, W, 3) uint8 image with H, W >= 1 and H W <= 2^29, "
                                 f"got {a.dtype} {tuple(a.shape)}")
            items.append((on_dev, a))
        # the host's images first, so that they are one run of the pool and one transfer
        order = [i for i, (d, _) in enumerate(items) if not d] + [i for i, (d, _) in enumerate(items) if d]
        shapes = [tuple(int(v) for v in a.shape[:2]) for _, a in items]
        offs, total = pool_layout([shapes[i] for i in order])
        offsets = [0] * len(items)
        for i, off in zip(order, offs):
            offsets[i] = off
        pool = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
        host_idx = [i for i in order if not items[i][0]]
        if host_idx:
            last = host_idx[-1]
            host_bytes = offsets[last] + 3 * shapes[last][0] * shapes[last][1]
            staging = torch.empty(host_bytes, dtype=torch.uint8, pin_memory=True)
            pack_images([items[i][1] for i in host_idx], staging.numpy())
            pool[:host_bytes].copy_(staging, non_blocking=True)
        for i in order:
            if items[i][0]:
                a = items[i][1]
                pool[offsets[i]:offsets[i] + a.numel()].view(a.shape).copy_(a)
        return pool, offsets, shapes

    def resample_ragged(self, images, boxes=None, size=None, flip=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype=None):
        """images: a list of (H, W, 3) u8 images of any sizes, NumPy arrays or torch tensors, on the
        host or on this device.  Box i = (oy, ox, bh, bw) of image i (boxes=None: each image whole;
        fit_boxes gives the usual ones), resized to size = (oh, ow) as resample_boxes resizes, bit
        for bit, mirrored where flip[i] is true, becomes image i of the result: (N, 3, oh, ow)
        torch.float32 (the default) or torch.float16 holding (v / 255 - mean[c]) / std[c], or
        (N, oh, ow, 3) torch.uint8.  One upload (upload_pool) and one launch on the current stream
        (nic_resample_ragged) for at most 65535 images.  Every row is checked here before the upload:
        ValueError naming the image or the row."""
        torch = _torch()
        who = "resample_ragged"
        if size is None:
            raise ValueError(f"{who}: size = (oh, ow) is required")
        dtype, kind, oh, ow, _, _ = self._resample_args(who, size, dtype, mean, std)
        if not (1 <= oh <= 16384 and 1 <= ow <= 16384):
            raise ValueError(f"{who}: size {oh} x {ow} not in 1..16384")
        images = list(images)
        n = len(images)
        if n > 65535:
            raise ValueError(f"{who}: {n} images in one call, at most 65535")
        flips = [0] * n if flip is None else [int(bool(f)) for f in flip]
        if len(flips) != n:
            raise ValueError(f"{who}: {len(flips)} flips for {n} images: one per image, or None")
        if boxes is not None:
            boxes = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes, dtype=np.int64).reshape(-1, 4) \
                if len(boxes) else np.zeros((0, 4), np.int64)
            if boxes.shape[0] != n:
                raise ValueError(f"{who}: {boxes.shape[0]} boxes for {n} images: one per image, or None")
        dev = torch.device("cuda", self.device)
        if n == 0:
            return torch.empty((0, oh, ow, 3) if kind == 2 else (0, 3, oh, ow), dtype=dtype, device=dev)
        # the shapes and the boxes first: nothing goes up for a call that is refused
        for i, a in enumerate(images):
            shape = tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape
            if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
                raise ValueError(f"{who}: image {i}: expected an (H, W, 3) uint8 image with H, W >= 1, got shape {shape}")
            if boxes is not None:
                oy, ox, bh, bw = boxes[i].tolist()
                if bh < 1 or bw < 1 or oy < 0 or ox < 0 or oy + bh > shape[0] or ox + bw > shape[1]:
                    raise ValueError(f"{who}: row {i}: a {bh} x {bw} box at ({oy}, {ox}) does not lie inside its "
                                     f"{shape[0]} x {shape[1]} image")
        pool, offsets, shapes = self.upload_pool(images)
        table = np.empty((n, 8), np.int64)
        table[:, 0] = offsets
        table[:, 1:3] = shapes
        table[:, 3:7] = boxes if boxes is not None else [(0, 0, h, w) for h, w in shapes]
        table[:, 7] = np.arange(n, dtype=np.int64) | (np.asarray(flips, np.int64) << 32)
        return self.resample_pool(pool, torch.from_numpy(table).to(dev), (oh, ow), dtype, mean, std, n_out=n)

    # -- device PNG writer (nic_png_device_*) -------------------------------------------------
    def png_reserve(self, n: int, h: int, w: int, channels: int = 3) -> None:
        """Grow the workspace so png_encode of n (h, w, channels) images allocates nothing."""
        _lib.check(self._L.nic_png_device_reserve(self._h, n, h, w, channels), "nic_png_device_reserve")

    def png_encode(self, x, filter="adaptive", stride: Optional[int] = None):
        """(N,H,W,3), (N,H,W,1) or (N,H,W) u8 device images -> (buf (N, stride) u8, sizes (N,)
        int64), device tensors: image i's complete PNG file is buf[i, :sizes[i]], written on the
        device (nic_png_device_encode; no host synchronisation).  filter: "adaptive" (Pillow's
        per-row choice) or 0..4 for one fixed PNG filter; stride: bytes between files, at least
        nic_png_device_bound (the default)."""
        torch = _torch()
        if isinstance(x, torch.Tensor) and x.ndim == 3:
            x = x.unsqueeze(-1)
        if not isinstance(x, torch.Tensor) or x.ndim != 4 or x.shape[3] not in (1, 3):
            raise ValueError("png_encode: expected an (N,H,W,3), (N,H,W,1) or (N,H,W) tensor")
        x = self._check_dev(x, 4, int(x.shape[3]), "png_encode")
        n, h, w, ch = x.shape
        if filter != "adaptive" and filter not in (0, 1, 2, 3, 4):
            raise ValueError(f"png_encode: filter must be 'adaptive' or 0..4, got {filter!r}")
        f = _lib.PNG_FILTER_ADAPTIVE if filter == "adaptive" else int(filter)
        bound = ctypes.c_int64()
        _lib.check(self._L.nic_png_device_bound(h, w, ch, ctypes.byref(bound)), "nic_png_device_bound")
        stride = bound.value if stride is None else int(stride)
        buf = torch.empty((n, stride), dtype=torch.uint8, device=x.device)
        sizes = torch.zeros((n,), dtype=torch.int64, device=x.device)
        _lib.check(self._L.nic_png_device_encode(self._h, x.data_ptr(), n, h, w, ch, f, buf.data_ptr(), stride,
                                                 sizes.data_ptr(), _stream_ptr(torch, self.device)), "nic_png_device_encode")
        return buf, sizes

    # -- device PNG reader (nic_png_device_read*) ---------------------------------------------
    def png_read_reserve(self, n: int, h: int, w: int, channels: int = 3) -> None:
        """Grow the workspace so png_read of n (h, w, channels) images allocates nothing."""
        _lib.check(self._L.nic_png_device_read_reserve(self._h, n, h, w, channels), "nic_png_device_read_reserve")

    def png_read_status(self, streams, sizes, h: int, w: int, channels: int = 3, out=None):
        """png_read without the check: (images, status (N,) int32 device tensor; bits in nic.h)."""
        torch = _torch()
        if (not isinstance(streams, torch.Tensor) or streams.dtype != torch.uint8 or streams.device.type != "cuda"
                or streams.ndim != 2):
            raise TypeError("png_read: expected an (N, stride) cuda torch.uint8 tensor of zlib streams")
        if not isinstance(sizes, torch.Tensor) or sizes.dtype != torch.int64 or sizes.shape != (streams.shape[0],):
            raise TypeError("png_read: expected an (N,) torch.int64 tensor of sizes")
        if streams.device.index != self.device or sizes.device != streams.device:
            raise ValueError(f"png_read: tensors must be on cuda:{self.device}")
        streams, sizes = streams.contiguous(), sizes.contiguous()
        n, stride = streams.shape
        shape = (n, int(h), int(w), int(channels))
        if out is None:
            out = torch.empty(tuple(max(v, 0) for v in shape), dtype=torch.uint8, device=streams.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != streams.device or not out.is_contiguous():
            raise TypeError("png_read: out must be a contiguous (N,h,w,channels) torch.uint8 tensor on the codec's device")
        status = torch.zeros((n,), dtype=torch.int32, device=streams.device)
        _lib.check(self._L.nic_png_device_read(self._h, streams.data_ptr(), stride, sizes.data_ptr(), n, int(h), int(w),
                                               int(channels), out.data_ptr(), status.data_ptr(),
                                               _stream_ptr(torch, self.device)), "nic_png_device_read")
        return out, status

    def png_read(self, streams, sizes, h: int, w: int, channels: int = 3, out=None):
        """The zlib streams streams[i, :sizes[i]] (device tensors: the IDAT payloads of PNG files of
        one (h, w, channels), bitstream.png_stream) -> ((N,h,w,channels) u8 images, status): inflated,
        Adler-checked and unfiltered on the device (nic_png_device_read).  Reads the statuses back
        (synchronises) and raises ValueError naming the first image whose stream did not decode."""
        images, status = self.png_read_status(streams, sizes, h, w, channels, out)
        st = status.cpu().numpy()
        bad = np.nonzero(st)[0]
        if bad.size:
            raise ValueError(f"png_read: image {int(bad[0])} is corrupt (status {int(st[bad[0]])}; corrupt images: "
                             f"{bad.tolist()})")
        return images, status

    def pack(self, z):
        """(N,h,w,96) -> (N,4h,8w,3) bitstream image (utils.py:39-40)."""
        torch = _torch()
        z = self._check_dev(z, 4, 96, "pack")
        n, h8, w8, _ = z.shape
        out = torch.empty((n, 4 * h8, 8 * w8, 3), dtype=torch.uint8, device=z.device)
        _lib.check(self._L.nic_pack_latent(z.data_ptr(), n, h8, w8, out.data_ptr(), _stream_ptr(torch, self.device)),
                   "nic_pack_latent")
        return out

    def unpack(self, img):
        """(N,4h,8w,3) -> (N,h,w,96) (utils.py:35-36)."""
        torch = _torch()
        img = self._check_dev(img, 4, 3, "unpack")
        n, hh, ww, _ = img.shape
        if hh % 4 or ww % 8:
            raise ValueError(f"unpack: packed image {tuple(img.shape)} is not (N,4h,8w,3)")
        out = torch.empty((n, hh // 4, ww // 8, 96), dtype=torch.uint8, device=img.device)
        _lib.check(self._L.nic_unpack_latent(img.data_ptr(), n, hh // 4, ww // 8, out.data_ptr(),
                                             _stream_ptr(torch, self.device)), "nic_unpack_latent")
        return out


class ProClass:
    """utils.py:15-62: shared Y/CbCr model holder (kind 'encoder' or 'decoder')."""

    #: chunks of the native host-array pipeline per call (nic_encode_host / nic_decode_host):
    #: 3 ramped chunks measured fastest for the config-2 batch (2.00 vs 2.07 ms for 4, 2.08 for
    #: 2; descending / ascending chunk sizes no better, profiles/r3n_host_plan_sweep.txt)
    host_chunks = 3

    kind = ""

    def __init__(self, device: Optional[int] = None, codec: Optional[Codec] = None, precision: str = "f16x3"):
        self.codec = codec if codec is not None else Codec(device, precision=precision)

    def load(self, path: str) -> None:
        """utils.py:26-28: weights from ``path + 'Y'`` and ``path + 'CbCr'`` (safetensors)."""
        self.codec.set_weights(W.load(path, self.kind))

    def set_weights(self, weights: W.Weights) -> None:
        sub = {k: v for k, v in weights.items() if k.startswith(self.kind)}
        W.validate(sub, [self.kind + m for m in W.PLANE_MODELS])
        self.codec.set_weights(sub)

    def _device_call(self, x):
        raise NotImplementedError

    def _host_call(self, a: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def __call__(self, x):
        """Device tensors stay on the device; host arrays (NumPy, CPU tensors) go through the
        native chunked host pipeline and come back as NumPy (in page-locked memory)."""
        torch = _torch()
        if isinstance(x, torch.Tensor) and x.device.type == "cuda":
            return self._device_call(x)
        a = _as_u8_array(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, type(self).__name__)
        if a.ndim != 4:
            raise ValueError(f"{type(self).__name__}: expected a 4-D NHWC batch, got shape {a.shape}")
        return self._host_call(a)


class Encoder(ProClass):
    """encoder.py:34-51."""

    kind = "encoder"

    def _device_call(self, x):
        return self.codec.encode(x)

    def _host_call(self, a):
        if a.shape[3] != 3:
            raise ValueError(f"Encoder: expected shape (N,H,W,3), got {a.shape}")
        return self.codec.encode_host(a, self.host_chunks)

    def encode_rdoq(self, x, lam: float, seg_pixels: int = 32):
        """(N,H,W,3) u8 on the device -> the latent whose codes are chosen by distortion + lam x bits
        under the codec's prior: encode(x, prequant=True), then Codec.rdoq (the context prior first).
        lam = 0 gives encode(x)'s codes."""
        z, f = self.codec.encode(x, prequant=True)
        return self.codec.rdoq(z, f, lam, seg_pixels)

    #: images per device batch of encode_resized: cut by count, since every batch has one shape
    resized_batch = 64

    def encode_resized(self, images, size, boxes=None, mode: str = "center"):
        """(H, W, 3) u8 images of any sizes (a list; NumPy or torch, host or device) -> their latents at
        one working size: box i of image i (default: fit_boxes(shapes, size, mode)) is resized to
        size = (oh, ow) on the device (Codec.resample_ragged to u8, rounded half to even) and encoded.
        (N, ceil(oh/8), ceil(ow/8), 96) u8 on the codec's device, in the images' order, equal to
        encode(resample_ragged(images, boxes, size, dtype=torch.uint8)).  The images go through the
        device ``resized_batch`` (64) at a time whatever their sizes: one upload, one resize launch and
        one encode per batch."""
        torch = _torch()
        images = list(images)
        try:
            oh, ow = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"encode_resized: size must be (oh, ow), got {size!r}") from None
        if boxes is None:
            shapes = []
            for i, a in enumerate(images):
                shape = tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape
                if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
                    raise ValueError(f"encode_resized: image {i}: expected an (H, W, 3) uint8 image with H, W >= 1, got shape {shape}")
                shapes.append(shape[:2])
            boxes = fit_boxes(shapes, (oh, ow), mode)
        elif len(boxes) != len(images):
            raise ValueError(f"encode_resized: {len(boxes)} boxes for {len(images)} images: one per image, or None")
        codec = self.codec
        h8, w8 = _lib.latent_shape(oh, ow)
        z = torch.empty((len(images), h8, w8, 96), dtype=torch.uint8, device=f"cuda:{codec.device}")
        for i in range(0, len(images), self.resized_batch):
            j = min(i + self.resized_batch, len(images))
            try:
                x = codec.resample_ragged(images[i:j], boxes[i:j], (oh, ow), dtype=torch.uint8)
            except ValueError as e:
                raise ValueError(f"encode_resized: images {i}..{j - 1}: {e}") from None
            codec.encode(x, out=z[i:j])
        return z

    def compress(self, dataset_path: str, checkpoint_path: str, batch_size: int = 64, workers=None,
                 container: str = "png", prior=None, png_reader: str = "pillow", resize=None,
                 resize_mode: str = "center", rdoq=None) -> None:
        """encoder.py:49-51: every image in ``dataset_path`` -> ``dataset_path + '_compressed'``.
        Pipelined over the host cores in batches of ``batch_size`` (bitstream.use_model);
        ``workers=0, batch_size=4`` is the reference's serial loop (same files).
        ``container="nic"`` writes ``<stem>.nic`` files, entropy-coded on the device, instead of
        the reference's packed PNGs (the default).  ``prior`` (a prior.Prior or a ``.nicp`` path;
        ``container="nic"`` only): version-2 files, coded against the prior and carrying each
        image's true H x W.  A prior.ContextPrior or a ``.nicc`` path: version-3 files, coded
        against the context prior.
        ``png_reader="device"``: the directory's PNG files are inflated and unfiltered on the device
        (Codec.png_read) instead of by Pillow on the reader pool; the files written are the same.
        ``resize=(oh, ow)``: every image, whatever its size, is first resized on the device to oh x ow
        from the box fit_boxes(..., resize_mode) gives it, and the directory goes through the device
        ``batch_size`` images at a time whatever their sizes (bitstream.use_model); version-2 and
        version-3 ``.nic`` files record oh x ow as the image's size.  Without it nothing changes.
        ``rdoq=lam`` (``container="nic"`` with a prior only, lam in [0, 16]; ValueError otherwise):
        every batch's codes are chosen by distortion + lam x bits under the prior the files are coded
        with (encode_rdoq) before they are coded; any ``.nic`` reader decodes the files.  Without it
        nothing changes, not even the launches."""
        from .bitstream import use_model

        more = {"png_reader": png_reader} if png_reader != "pillow" else {}
        if resize is not None:
            more.update(resize=resize, resize_mode=resize_mode)
        if rdoq is not None:
            more["rdoq"] = rdoq
        use_model(self, dataset_path, checkpoint_path, dataset_path + "_compressed", in_cshape=3,
                  batch_size=batch_size, workers=workers, container=container, prior=prior, **more)


class Decoder(ProClass):
    """decoder.py:35-52."""

    kind = "decoder"

    def _device_call(self, z):
        return self.codec.decode(z)

    def _host_call(self, a):
        if a.shape[3] != 96:
            raise ValueError(f"Decoder: expected shape (N,h,w,96), got {a.shape}")
        return self.codec.decode_host(a, self.host_chunks)

    def decode_region(self, files, box):
        """The pixel box = (y, x, h, w) of the images of .nic files (bytes or paths, one latent shape)
        -> (N,h,w,3) u8 device tensor, equal to that box of the whole reconstructions: only the
        segments and the latent window the box needs are decoded (bitstream.decode_region)."""
        from .bitstream import decode_region

        return decode_region(self, files, box)

    def decode_regions(self, files, boxes):
        """One pixel box (y, x, h, w) per .nic file, all of one (h, w), out of files whose images may
        differ in size: an (N,h,w,3) u8 tensor on this device, in the files' order, each equal to the
        box cut out of that file's whole reconstruction.  The windows of one call have one shape, so
        files of different frames are entropy-decoded and run through the decoder as one batch
        (bitstream.decode_regions)."""
        from .bitstream import decode_regions

        return decode_regions(self, files, boxes)

    def decode_crops(self, files, boxes, size, flip=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype=None, bucket=None):
        """One pixel box (y, x, h, w) per .nic file, the boxes of any sizes, each resized to size =
        (oh, ow) (bilinear, antialiased), mirrored where flip[i] is true, normalised with mean and std
        and laid out for a model: (N, 3, oh, ow) torch.float32 (the default) or torch.float16, or
        (N, oh, ow, 3) torch.uint8, on this device, in the files' order -- what RandomResizedCrop,
        a flip, ToTensor and Normalize give, from the files' bytes, in one call
        (bitstream.decode_crops)."""
        from .bitstream import decode_crops

        return decode_crops(self, files, boxes, size, flip=flip, mean=mean, std=std, dtype=dtype, bucket=bucket)

    def uncompress(self, dataset_path: str, checkpoint_path: str, batch_size: int = 64, workers=None,
                   container: str = "png", png_writer: str = "pillow", prior=None, region=None,
                   png_reader: str = "pillow") -> None:
        """decoder.py:50-52: packed PNGs in ``dataset_path`` -> ``dataset_path.replace('compressed','uncompressed')``.
        Pipelined as compress (``workers=0, batch_size=4``: the reference's serial loop).
        ``container="nic"`` reads the directory's ``.nic`` files instead (same reconstructions).
        ``png_writer="device"`` writes the reconstructions with the device PNG writer (the same
        pixels in files of its own format) instead of Pillow's optimize=True bytes.
        ``prior`` (``container="nic"`` only): the prior the directory's version-2 files were written
        under (a prior.ContextPrior or a ``.nicc`` path for version-3 files); their reconstructions
        are cropped to the recorded H x W.  Version-1 files are read as before.
        ``region`` (a pixel box (y, x, h, w); ``container="nic"`` only, ValueError otherwise: a packed
        PNG has no index): every file is decoded to that box only and ``<stem>.png`` holds the box.
        ``png_reader="device"`` (``container="png"`` only, ValueError otherwise): the packed PNGs are
        inflated and unfiltered on the device (Codec.png_read) and go straight into the unpack."""
        from .bitstream import use_model

        more = {"region": region} if region is not None else {}
        if png_reader != "pillow":
            more["png_reader"] = png_reader
        use_model(self, dataset_path, checkpoint_path, dataset_path.replace("compressed", "uncompressed"),
                  in_cshape=96, batch_size=batch_size, workers=workers, container=container, png_writer=png_writer,
                  prior=prior, **more)
