"""The instrument of tests/test_gpu_stream_contract.py: a gate that holds a torch side stream for a
known time, a sentinel arena that every device buffer a wrapper allocates comes out of, and the two
protocols (asynchronous entry points; documented synchronising ones).  DESIGN.md section 24.

A gate is torch.cuda._sleep on a torch.cuda.Stream() with an event recorded behind it.  Torch's side
streams are non-blocking, so work that a call puts on the null stream does not wait for the gate: it
runs at once, while the inputs still hold the decoy and the outputs the sentinel.

What one asynchronous case asserts (run_async):
  no host synchronisation   the gate's event is still pending when the call returns
  nothing ran early         a copy taken on a third stream while the gate is pending shows every
                            buffer the call allocated, outputs included, still all sentinel
  on the stream, in order   after the stream is drained every output equals, byte for byte, what the
                            same call gave on the default stream
"""
import contextlib
import time

import torch

SENTINEL_BYTE = 0xA5
GATE_MIN_MS = 200.0   # the least a gate holds its stream
GATE_HOST_FACTOR = 50  # ... or this many times the warm call's host time
GATE_MAX_MS = 1000.0
HOST_MAX_MS = 20.0    # a warm call that keeps the host longer fails its case; the gate is not lengthened
ARENA_BYTES = 32 << 20

# Wrappers that synchronise by their own words and are NOT gated.  Each entry: the wrapper, and the
# fragments of the sentence (codec.py's docstring or nic.h, as they stood before these tests) that
# says so; test_synchronising_list_quotes_the_sources looks each fragment up in those two files.  A
# wrapper may stand here only with such a sentence; anything else that synchronises is a finding.
SYNCHRONISING_UNGATED = {
    "Codec.rans_decode / rans2_decode / rans3_decode":
        ("Reads the statuses back (synchronises) and raises ValueError naming the first image whose file did not decode cleanly.",),
    "Codec.rans_decode_window / rans2_decode_window / rans3_decode_window":
        ("Reads the statuses back (synchronises) and raises ValueError naming the first image that did not decode cleanly",),
    "Codec.rans_decode_windows / rans2_decode_windows / rans3_decode_windows":
        ("Reads the statuses back (synchronises) and raises ValueError naming the first image that was refused or did not decode cleanly.",),
    "Codec.png_read":
        ("Reads the statuses back (synchronises) and raises ValueError naming the first image whose stream did not decode.",),
    "Codec.cut_boxes / resample_boxes / *_decode_windows* with a host table":
        ("offsets: N pairs of host integers, checked here against the images (ValueError naming the row) and uploaded",
         "table: N rows of host integers, checked here against the images and n_out (ValueError naming the row) and uploaded",
         "table: N rows of host integers, uploaded here"),
    "Codec.resample_ragged / upload_pool / Encoder.encode_resized":
        ("Every row is checked here before the upload",),
    "Codec.set_tensor / set_weights (nic_set_weights)": ("The kernel is repacked to the device-native fragment layout. Synchronous.",),
    "Codec.reserve / rans*_reserve / png_reserve / png_read_reserve":
        ("Grow the workspace so encode of (n, h, w) images and decode of their latents allocate nothing. Synchronous.",
         "latents allocate nothing. Synchronous.", "allocates nothing. Synchronous."),
}
# Synchronising wrappers that had NO such sentence before these tests: findings.  Each now has one
# (the fragment below, added to its docstring with this work) and is recorded in DESIGN section 24.
SYNCHRONISING_FOUND = {
    "Codec.psnr": ("Reads the sums back to the host (synchronises).",),
}
# The gated ones, with their sentences (test_gpu_stream_contract.SYNC_CASES asserts the opposite of
# the asynchronous cases: the call must not return before the gate ends).
SYNCHRONISING_GATED = {
    "encode_host": "the call is ordered after the work queued on `stream` and returns with the outputs written (synchronous)",
    "decode_host": "the call is ordered after the work queued on `stream` and returns with the outputs written (synchronous)",
    "set_prior": "nic_rans_prior_set: ... Synchronous (waits for the device).",
    "set_context_prior": "nic_rans_cprior_set: ... Synchronous.",
    "range_trips": "nic_range_trips (synchronising) counts the passes that tripped since nic_create.",
    "layer_times": "Both synchronise on the recorded events.",
    "encode_range_error": "NIC_RANGE_ERROR -- the call synchronises its stream after the split pass",
}


def fill_sentinel(t):
    t.view(torch.uint8).fill_(SENTINEL_BYTE)
    return t


def as_bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(as_bytes(a), as_bytes(b))


class Gate:
    """Calibrated once: device cycles of torch.cuda._sleep per millisecond, and three streams of
    which `side` and `other` can be held while `third` and the default stream still run (the machine
    may map several streams onto one hardware queue; such streams could not show an early launch)."""

    def __init__(self, device=0):
        if not hasattr(torch.cuda, "_sleep"):
            raise RuntimeError("torch.cuda._sleep is missing: the gate needs a matmul chain sized by the same calibration")
        self.device = device
        self.cycles_per_ms = self._calibrate()
        self.side, self.third, self.other = self._pick_streams()
        self.log = {}  # case id -> (warm host ms, gate ms)

    def _calibrate(self):
        best = None
        for cycles in (1_000_000, 20_000_000, 20_000_000):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            best = cycles / max(a.elapsed_time(b), 1e-3)
        return best

    def hold(self, stream, ms):
        """Keeps `stream` busy for ms; the event behind the gate."""
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(ms * self.cycles_per_ms))
            ev = torch.cuda.Event()
            ev.record(stream)
        return ev

    def _runs_beside(self, held, others):
        """True when a small kernel on each of `others` (None: the default stream) finishes while
        every stream of `held` is gated."""
        probe = torch.zeros(64, device=f"cuda:{self.device}")
        torch.cuda.synchronize()
        evs = [self.hold(h, 40.0) for h in held]
        ok = True
        for s in others:
            with torch.cuda.stream(s) if s is not None else contextlib.nullcontext():
                probe.add_(1.0)
            (s if s is not None else torch.cuda.default_stream(self.device)).synchronize()
            ok = ok and not any(ev.query() for ev in evs)
        torch.cuda.synchronize()
        return ok

    def _pick_streams(self):
        """side, third, other: with side and other both held (the two-stream case holds both), the
        default stream and third still run."""
        pool = [torch.cuda.Stream(self.device) for _ in range(8)]
        side = next((s for s in pool if self._runs_beside([s], [None])), None)
        other = None if side is None else next((s for s in pool if s is not side and self._runs_beside([side, s], [None])), None)
        third = None if other is None else next((s for s in pool if s is not side and s is not other
                                and self._runs_beside([side, other], [None, s])), None)
        if third is None:
            raise RuntimeError("no two side streams can be held while the default stream and a third stream run")
        return side, third, other

    def size(self, host_ms):
        return min(GATE_MAX_MS, max(GATE_MIN_MS, GATE_HOST_FACTOR * host_ms))


class Arena:
    """Device buffers for everything a wrapper allocates with torch.empty / empty_like / zeros while
    the arena is open: slices of one slab that was filled with the sentinel before the gate, so a
    buffer is all sentinel until work on the gated stream writes it.  (A fill inside the call would
    itself wait behind the gate.)  Host and pinned allocations pass through."""

    def __init__(self, device):
        self.device = torch.device("cuda", device)
        self.slab = fill_sentinel(torch.empty(ARENA_BYTES, dtype=torch.uint8, device=self.device))
        self.used = 0
        self._real = self._mine = None
        self._empty = torch.empty

    def reset(self):
        """Back to all sentinel and nothing handed out (on the current stream; the caller synchronises)."""
        if self.used:
            fill_sentinel(self.slab[:self.used])
        self.used = 0

    def take(self, shape, dtype):
        shape = tuple(int(v) for v in shape)
        n = 1
        for v in shape:
            n *= v
        nbytes = n * self._empty((), dtype=dtype).element_size()
        at = self.used
        self.used = (at + nbytes + 255) & ~255
        if self.used > ARENA_BYTES:
            raise RuntimeError(f"the sentinel arena of {ARENA_BYTES} bytes is too small for this case")
        # its own tensor on the slab's storage, not a view: autograd's version counters stay apart
        t = self._empty(0, dtype=dtype, device=self.device)
        return t.set_(self.slab.untyped_storage(), at // t.element_size(), shape)

    def _is_dev(self, kw):
        dev = kw.get("device")
        if dev is None or kw.get("pin_memory"):
            return False
        return torch.device(dev).type == "cuda"

    @contextlib.contextmanager
    def open(self):
        real = torch.empty, torch.empty_like, torch.zeros

        def shape_of(args, kw):
            if "size" in kw:
                args = (kw["size"],)
            return tuple(args[0]) if len(args) == 1 and not isinstance(args[0], int) else args

        def empty(*args, **kw):
            if not self._is_dev(kw):
                return real[0](*args, **kw)
            return self.take(shape_of(args, kw), kw.get("dtype") or torch.float32)

        def empty_like(t, **kw):
            if not t.is_cuda or kw:
                return real[1](t, **kw)
            return self.take(t.shape, t.dtype)

        def zeros(*args, **kw):
            if not self._is_dev(kw):
                return real[2](*args, **kw)
            return self.take(shape_of(args, kw), kw.get("dtype") or torch.float32).zero_()

        self._real, self._mine = real, (empty, empty_like, zeros)
        torch.empty, torch.empty_like, torch.zeros = self._mine
        try:
            yield self
        finally:
            torch.empty, torch.empty_like, torch.zeros = real
            self._real = self._mine = None

    @contextlib.contextmanager
    def paused(self):
        """Ordinary allocations inside an open arena, for objects that outlive the case's call."""
        mine = self._mine
        if mine is not None:
            torch.empty, torch.empty_like, torch.zeros = self._real
        try:
            yield
        finally:
            if mine is not None:
                torch.empty, torch.empty_like, torch.zeros = mine

    def holds(self, t):
        """Does t lie inside the bytes handed out so far?"""
        base = self.slab.data_ptr()
        return t.numel() > 0 and base <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= base + self.used

    def untouched(self, stream):
        """On `stream`: is every byte handed out so far still the sentinel?"""
        with torch.cuda.stream(stream):
            ok = (self.slab[:self.used] == SENTINEL_BYTE).all() if self.used else torch.ones((), dtype=torch.bool, device=self.device)
        stream.synchronize()
        return bool(ok.item())


def _clone_all(ts):
    return [t.clone() for t in ts]


def _outputs(res):
    if isinstance(res, torch.Tensor):
        return [res]
    return [t for t in res if t is not None]


def expected_on_default_stream(make, call):
    """Steps 1 and 2: decoy A and real B, their results on the default stream (no arena: ordinary
    buffers), and the assertion that the two differ in every output array."""
    a, b = make("A"), make("B")
    assert len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a, b)), "A and B differ in shape"
    exp_a = _clone_all(_outputs(call(_clone_all(a))))
    exp_b = _clone_all(_outputs(call(_clone_all(b))))
    torch.cuda.synchronize()
    assert len(exp_a) == len(exp_b) and exp_b
    for i, (x, y) in enumerate(zip(exp_a, exp_b)):
        assert x.numel() and not same_bytes(x, y), f"output {i}: decoy A and real B give the same bytes; the case cannot tell them apart"
    return a, b, exp_b


def _warm(gate, arena, call, inp, name):
    """Step 4: two ungated runs on the idle side stream (the first takes whatever the call sets up
    once); the second one's host time sizes the gate."""
    host_ms = 0.0
    for _ in range(2):
        arena.reset()
        torch.cuda.synchronize()
        with torch.cuda.stream(gate.side), arena.open():
            t0 = time.perf_counter()
            call(inp)
            host_ms = (time.perf_counter() - t0) * 1e3
        gate.side.synchronize()
    assert host_ms <= HOST_MAX_MS, f"{name}: the warm call keeps the host {host_ms:.2f} ms (limit {HOST_MAX_MS} ms)"
    return host_ms


def run_async(gate, arena, name, make, call, reserve=None, outside=0):
    """The protocol for one entry point that promises "on `stream`, no host synchronisation".
    make(which) -> the list of input tensors for which = "A" or "B"; call(inputs) -> output tensor(s),
    reading only `inputs` (in-out tensors are inputs that the call also returns).
    Every output must lie in the sentinel arena or be one of the live inputs (written in place), so
    that the sentinel check is about the buffers the results are in; `outside`: how many outputs may
    lie elsewhere because torch computes them, in stream order, from buffers that do (a masked file
    buffer, a dtype conversion, an autograd sum).  Returns the gated call's outputs (clones)."""
    a, b, exp_b = expected_on_default_stream(make, call)
    if reserve is not None:
        reserve()
    inp = _clone_all(a)
    torch.cuda.synchronize()
    host_ms = _warm(gate, arena, call, inp, name)
    gate_ms = gate.size(host_ms)
    gate.log[name] = (host_ms, gate_ms)
    for t, src in zip(inp, a):
        t.copy_(src)
    arena.reset()
    torch.cuda.synchronize()
    ev = gate.hold(gate.side, gate_ms)
    with torch.cuda.stream(gate.side), arena.open():
        for t, src in zip(inp, b):
            t.copy_(src)  # the inputs do not exist until the gate ends
        outs = _outputs(call(inp))
    returned_early = not ev.query()
    with torch.cuda.stream(gate.side):
        got = _clone_all(outs)
    live = {t.data_ptr() for t in inp}
    stray = [i for i, t in enumerate(outs) if not arena.holds(t) and t.data_ptr() not in live]
    in_place = all(t.data_ptr() in live for t in outs)
    clean = arena.untouched(gate.third)
    still_held = not ev.query()
    gate.side.synchronize()
    print(f"[stream-contract] {name}: warm host {host_ms:.3f} ms, gate {gate_ms:.0f} ms, arena {arena.used} B")
    assert returned_early, f"{name}: the call returned only after the {gate_ms:.0f} ms gate had ended: it synchronises the host"
    assert still_held, f"{name}: gate too short: its {gate_ms:.0f} ms ended before the sentinel check was read"
    assert clean, f"{name}: a buffer of the call was written while the gate still held the stream: work ran off the stream"
    assert len(stray) <= outside, f"{name}: outputs {stray} lie neither in the sentinel arena nor in the inputs ({outside} allowed): " \
        "the wrapper allocates in a way the arena does not see, and the sentinel check would not cover them"
    assert arena.used > 0 or in_place or stray, f"{name}: the call allocated nothing from the sentinel arena"
    assert len(got) == len(exp_b)
    for i, (x, y) in enumerate(zip(got, exp_b)):
        assert same_bytes(x, y), f"{name}: output {i} differs from the default-stream result: work ran off the stream or out of order"
    return got


def run_sync(gate, name, call, check, setup=None, warm=True):
    """A documented synchronising call behind a gate: it must not return before the gate ends, and
    must still give the right results.  setup(): queued on the gated side stream before the call;
    call() -> result, run with the side stream current; check(result) asserts it."""
    if warm:
        with torch.cuda.stream(gate.side):
            call()
        gate.side.synchronize()
    torch.cuda.synchronize()
    ev = gate.hold(gate.side, GATE_MIN_MS)
    with torch.cuda.stream(gate.side):
        if setup is not None:
            setup()
        res = call()
    waited = ev.query()
    gate.side.synchronize()
    assert waited, f"{name}: returned while the gate still held the stream: it did not wait for the work queued there"
    check(res)
