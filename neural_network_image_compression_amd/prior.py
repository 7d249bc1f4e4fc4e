"""The codec-level prior of the .nic container's version 2 ("The .nic container,
version 2"): the entropy model fitted once over a corpus, stored beside the weights and shared
by every file, so a file carries a table only for the channels where its own pays for itself.

    acc = Prior.accumulator(codec)
    for batch in corpus:
        acc.add(codec.encode(batch))      # counted on the device
    prior = acc.build()                   # normalised on the device
    prior.save("model.nicp")
    codec.set_prior(Prior.load("model.nicp"))

A ``.nicp`` file (49,168 B): ``NICP``, u8 version 1, u8 probability bits 12, u16 channels 96,
u32 prior_id, u32 zero, then the 96 x 256 freqs as little-endian u16, channel-major.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _lib

MAGIC = b"NICP"
CHANNELS = 96
FILE_BYTES = 16 + CHANNELS * 256 * 2


def check_freqs(freqs: np.ndarray) -> int:
    """The id of (96, 256) u16 freqs; ValueError (nic_rans_prior_check's text) if they break the
    invariants.  Host only."""
    pid = ctypes.c_uint32()
    rc = _lib.lib().nic_rans_prior_check(freqs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pid))
    if rc != _lib.NIC_OK:
        raise ValueError(f"[{rc}] {_lib.last_error()}")
    return int(pid.value)


class Prior:
    """96 x 256 freqs, each in 1..4096, every channel summing to 4096, and their id."""

    def __init__(self, freqs):
        a = np.asarray(freqs)
        if a.shape != (CHANNELS, 256) or a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 65535:
            raise ValueError(f"Prior: expected (96, 256) integer freqs in 1..4096, got shape {a.shape} dtype {a.dtype}")
        self.freqs = np.ascontiguousarray(a, dtype=np.uint16)
        self.freqs.setflags(write=False)
        self.id = check_freqs(self.freqs)

    def __eq__(self, other):
        return isinstance(other, Prior) and np.array_equal(self.freqs, other.freqs)

    def __hash__(self):
        return self.id

    def __repr__(self):
        return f"Prior(id={self.id:08x})"

    def to_bytes(self) -> bytes:
        return MAGIC + struct.pack("<BBHII", 1, 12, CHANNELS, self.id, 0) + self.freqs.astype("<u2").tobytes()

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, data: bytes, what: str = ".nicp") -> "Prior":
        if len(data) != FILE_BYTES or data[:4] != MAGIC:
            raise ValueError(f"{what}: not a .nicp file ({len(data)} bytes, expected {FILE_BYTES} starting with NICP)")
        ver, bits, ch, pid, zero = struct.unpack("<BBHII", data[4:16])
        if (ver, bits, ch, zero) != (1, 12, CHANNELS, 0):
            raise ValueError(f"{what}: unsupported .nicp header (version {ver}, {bits} bits, {ch} channels)")
        try:
            p = cls(np.frombuffer(data, "<u2", offset=16).reshape(CHANNELS, 256))
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
        if p.id != pid:
            raise ValueError(f"{what}: the header's prior_id {pid:08x} is not the freqs' {p.id:08x}")
        return p

    @classmethod
    def load(cls, path: str) -> "Prior":
        with open(path, "rb") as f:
            return cls.from_bytes(f.read(), path)

    @staticmethod
    def accumulator(codec) -> "PriorAccumulator":
        return PriorAccumulator(codec)


PSEUDO_COUNT_BITS = 40  # from_probabilities: a row's probabilities as counts out of 2^40


def pseudo_counts(p) -> np.ndarray:
    """(96, 256) probabilities -> the int64 pseudo-counts rint(p 2^40) that from_probabilities
    normalises (and nic_rans_prior_build normalises to the same freqs)."""
    a = np.asarray(p, dtype=np.float64)
    if a.shape != (CHANNELS, 256) or not np.all(np.isfinite(a)) or a.min() < 0 or \
            np.abs(a.sum(axis=1) - 1.0).max() > 1e-6:
        raise ValueError("from_probabilities: expected (96, 256) probabilities, every row summing to 1")
    return np.rint(a * float(1 << PSEUDO_COUNT_BITS)).astype(np.int64)


def _normalise(counts: np.ndarray) -> np.ndarray:
    """Rows of int64 counts -> freqs by nic_rans_prior_build's rule (from_probabilities states it)."""
    freqs = np.empty(counts.shape, np.int64)
    for r, c in enumerate(counts):
        n = int(c.sum())
        f = np.maximum(1, (c << 12) // n) if n else np.full(256, 16, np.int64)  # c 4096 < 2^53
        diff = 4096 - int(f.sum())
        if diff > 0:
            f[np.argmax(f)] += diff  # argmax: the lowest symbol on ties
        for _ in range(-diff):
            f[np.argmax(f)] -= 1
        freqs[r] = f
    return freqs


def from_probabilities(p) -> Prior:
    """A Prior from a (96, 256) float64 table of probabilities (a trained table's softmax,
    training.Training.prior): pseudo-counts c = rint(p 2^40), normalised on the host by the rule of
    nic_rans_prior_build: f = max(1, floor(4096 c / N)) with N the row's count;
    a deficit goes onto the largest entry, a surplus is taken one at a time from the currently
    largest entry, the lowest symbol on ties; N = 0 gives 16 everywhere."""
    return Prior(_normalise(pseudo_counts(p)))


def as_prior(prior):
    """A Prior from a Prior or a .nicp path (None stays None)."""
    if prior is None or isinstance(prior, Prior):
        return prior
    return Prior.load(str(prior))


class PriorAccumulator:
    """Counts of device latents in one uint64[96 * 256] device accumulator (nic_rans_prior_count:
    deterministic, no host synchronisation), normalised on the device (nic_rans_prior_build)."""

    def __init__(self, codec):
        import torch

        self.codec = codec
        # the 64-bit counts live in an int64 tensor (the same bits; a count stays far below 2^63)
        self.counts = torch.zeros((CHANNELS, 256), dtype=torch.int64, device=f"cuda:{codec.device}")

    def add(self, z) -> "PriorAccumulator":
        """Adds the counts of the latents z (N,h,w,96), a u8 tensor on the codec's device."""
        self.codec.prior_count(z, self.counts)
        return self

    def build(self) -> Prior:
        return Prior(self.codec.prior_build(self.counts).cpu().numpy())


# ---- version 3: the context prior ("The .nic container, version 3") -----------------
#
#     static = Prior.accumulator(codec) ... .build()            # first pass: the anchors' source
#     acc = ContextPrior.accumulator(codec, static)
#     for batch in corpus:
#         acc.add(codec.encode(batch))                           # second pass, counted on the device
#     cprior = acc.build()
#     cprior.save("model.nicc")
#     codec.set_context_prior(ContextPrior.load("model.nicc"))
#
# A ``.nicc`` file (147,568 B): ``NICC``, u8 version 1, u8 probability bits 12, u16 channels 96,
# u32 prior_id, u8 contexts 3, three zero bytes, the 96 anchors, then the 96 x 3 x 256 freqs as
# little-endian u16, channel-major, then context, then symbol.

CMAGIC = b"NICC"
CONTEXTS = 3
CFILE_BYTES = 16 + CHANNELS + CHANNELS * CONTEXTS * 256 * 2


def check_context_freqs(anchors: np.ndarray, freqs: np.ndarray) -> int:
    """The id of (96,) u8 anchors and (96, 3, 256) u16 freqs; ValueError (nic_rans_cprior_check's
    text, which names the channel and the context) if they break the invariants.  Host only."""
    pid = ctypes.c_uint32()
    rc = _lib.lib().nic_rans_cprior_check(anchors.ctypes.data_as(ctypes.c_void_p), freqs.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.byref(pid))
    if rc != _lib.NIC_OK:
        raise ValueError(f"[{rc}] {_lib.last_error()}")
    return int(pid.value)


class ContextPrior:
    """96 anchors and 96 x 3 x 256 freqs, each in 1..4096, every (channel, context) row summing to
    4096, and their id."""

    def __init__(self, anchors, freqs):
        a, f = np.asarray(anchors), np.asarray(freqs)
        if a.shape != (CHANNELS,) or a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 255:
            raise ValueError(f"ContextPrior: expected 96 integer anchors in 0..255, got shape {a.shape} dtype {a.dtype}")
        if f.shape != (CHANNELS, CONTEXTS, 256) or f.dtype.kind not in "iu" or f.min() < 0 or f.max() > 65535:
            raise ValueError(f"ContextPrior: expected (96, 3, 256) integer freqs in 1..4096, got shape {f.shape} dtype {f.dtype}")
        self.anchors = np.ascontiguousarray(a, dtype=np.uint8)
        self.freqs = np.ascontiguousarray(f, dtype=np.uint16)
        self.anchors.setflags(write=False)
        self.freqs.setflags(write=False)
        self.id = check_context_freqs(self.anchors, self.freqs)

    def __eq__(self, other):
        return (isinstance(other, ContextPrior) and np.array_equal(self.anchors, other.anchors)
                and np.array_equal(self.freqs, other.freqs))

    def __hash__(self):
        return self.id

    def __repr__(self):
        return f"ContextPrior(id={self.id:08x})"

    def to_bytes(self) -> bytes:
        return (CMAGIC + struct.pack("<BBHIB3x", 1, 12, CHANNELS, self.id, CONTEXTS) + self.anchors.tobytes()
                + self.freqs.astype("<u2").tobytes())

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, data: bytes, what: str = ".nicc") -> "ContextPrior":
        if len(data) != CFILE_BYTES or data[:4] != CMAGIC:
            raise ValueError(f"{what}: not a .nicc file ({len(data)} bytes, expected {CFILE_BYTES} starting with NICC)")
        ver, bits, ch, pid, ctx, zero = struct.unpack("<BBHIB3s", data[4:16])
        if (ver, bits, ch, ctx, zero) != (1, 12, CHANNELS, CONTEXTS, b"\0\0\0"):
            raise ValueError(f"{what}: unsupported .nicc header (version {ver}, {bits} bits, {ch} channels, {ctx} contexts, "
                             f"reserved {zero.hex()})")
        try:
            p = cls(np.frombuffer(data, np.uint8, CHANNELS, 16),
                    np.frombuffer(data, "<u2", offset=16 + CHANNELS).reshape(CHANNELS, CONTEXTS, 256))
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
        if p.id != pid:
            raise ValueError(f"{what}: the header's prior_id {pid:08x} is not the anchors' and freqs' {p.id:08x}")
        return p

    @classmethod
    def load(cls, path: str) -> "ContextPrior":
        with open(path, "rb") as f:
            return cls.from_bytes(f.read(), path)

    @staticmethod
    def accumulator(codec, static_prior: Prior, seg_pixels: int = 32) -> "ContextPriorAccumulator":
        return ContextPriorAccumulator(codec, static_prior, seg_pixels)


def anchors_of(static_prior: Prior) -> np.ndarray:
    """The anchor of every channel: the argmax of its row of a static prior, the lowest symbol on ties."""
    return np.argmax(static_prior.freqs, axis=1).astype(np.uint8)


def load_any(path: str):
    """A Prior or a ContextPrior from a .nicp / .nicc file, by its magic."""
    with open(path, "rb") as f:
        data = f.read()
    return ContextPrior.from_bytes(data, path) if data[:4] == CMAGIC else Prior.from_bytes(data, path)


def as_any_prior(prior):
    """A Prior or ContextPrior from either, or from a .nicp / .nicc path (None stays None)."""
    if prior is None or isinstance(prior, (Prior, ContextPrior)):
        return prior
    return load_any(str(prior))


class ContextPriorAccumulator:
    """Context counts of device latents in one uint64[96 * 3 * 256] device accumulator
    (nic_rans_cprior_count: deterministic, no host synchronisation), normalised on the device
    (nic_rans_cprior_build).  The counts depend on seg_pixels: a segment's first pixel is context 0."""

    def __init__(self, codec, static_prior: Prior, seg_pixels: int = 32):
        import torch

        if not isinstance(static_prior, Prior):
            raise TypeError("ContextPrior.accumulator: static_prior must be a prior.Prior (the anchors are its rows' argmax)")
        self.codec = codec
        self.seg_pixels = int(seg_pixels)
        self.anchors = anchors_of(static_prior)
        dev = f"cuda:{codec.device}"
        self._anchors_dev = torch.from_numpy(self.anchors.copy()).to(dev)
        self.counts = torch.zeros((CHANNELS, CONTEXTS, 256), dtype=torch.int64, device=dev)

    def add(self, z) -> "ContextPriorAccumulator":
        """Adds the context counts of the latents z (N,h,w,96), a u8 tensor on the codec's device."""
        self.codec.cprior_count(z, self._anchors_dev, self.counts, self.seg_pixels)
        return self

    def build(self) -> ContextPrior:
        return ContextPrior(self.anchors, self.codec.cprior_build(self.counts).cpu().numpy())


def context_pseudo_counts(p) -> np.ndarray:
    """(96, 3, 256) probabilities -> the int64 pseudo-counts rint(p 2^40) that
    context_from_probabilities normalises (and nic_rans_cprior_build normalises to the same freqs)."""
    a = np.asarray(p, dtype=np.float64)
    if a.shape != (CHANNELS, CONTEXTS, 256) or not np.all(np.isfinite(a)) or a.min() < 0 or \
            np.abs(a.sum(axis=2) - 1.0).max() > 1e-6:
        raise ValueError("context_from_probabilities: expected (96, 3, 256) probabilities, every row summing to 1")
    return np.rint(a * float(1 << PSEUDO_COUNT_BITS)).astype(np.int64)


def context_from_probabilities(anchors, p) -> ContextPrior:
    """A ContextPrior from 96 anchors and a (96, 3, 256) float64 table of probabilities (a trained
    context table's softmax, training.Training.context_prior): from_probabilities' pseudo-count
    rule applied to every (channel, context) row."""
    counts = context_pseudo_counts(p)
    return ContextPrior(anchors, _normalise(counts.reshape(-1, 256)).reshape(CHANNELS, CONTEXTS, 256))
