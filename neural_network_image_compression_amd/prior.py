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
