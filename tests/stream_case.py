"""Late inputs on a non-default stream (helper of tests/test_gpu_streams.py; a plain module).

Every other GPU test calls the library on torch's default stream with inputs that are complete
and synchronised.  A launch on the wrong stream, a side stream that does not wait, or an event
recorded on the wrong stream then reads the right bytes anyway.  Here the bytes are wrong until
late:

1. The true inputs are built on the CPU; the references are computed from these.
2. Every device-resident or pinned buffer the library will read is first filled with POISON (a
   finite sentinel, -7 in the buffer's dtype: a stale read changes bits, never makes a NaN).  The
   true values wait in separate staging tensors on the device.  One ``torch.cuda.synchronize()``.
3. Under ``s = torch.cuda.Stream()`` a DELAY is enqueued (in-place adds over a buffer of 256 MiB,
   ordinary torch work), an event is recorded behind it, and only then the copies that overwrite
   the poison with the true values (``copy_`` from the staging tensors).
4. Still under ``s`` the library is called; then ``s.synchronize()`` and the bitwise comparison.
5. Work of the library's that is not ordered behind ``s`` -- a launch on the null stream, a side
   stream that does not wait for ``s``, a readback that does not wait -- runs while the delay still
   holds ``s`` and sees poison (torch's streams are non-blocking: the null stream does not wait for
   them).
6. Non-vacuity: right after an asynchronous entry point returns, the event behind the delay must
   not have fired (``Late.call()``).  If it has, the delay was too short and the test FAILS; it never
   passes on luck.  Entry points that synchronise by contract pass ``sync="<the documented
   synchronisation>"`` and skip this one assertion.
7. ``Late.reuse``: still under ``s`` the test drops its device inputs and allocates and poisons
   tensors of the same sizes on ``s``.  Legal by stream semantics: the caching allocator hands the
   same blocks back at once unless ``record_stream`` told it of a reader on another stream.  A
   side-stream read without ``record_stream`` would then see poison -- but only if that read is
   still pending, so this check detects such a fault SOMETIMES, not always.

``Late(delay, ready=True)`` is the same case with everything ready on the default stream (what the
rest of the suite does): the tests assert both give the same bits, and the host-side issue time of
each library call is taken there (``ISSUE_MS``).

Delay length.  Measured on an MI355X (a full session of tests/test_gpu_streams.py, ``ready`` mode,
``time.perf_counter`` around each library call on an idle stream, 79 calls): median 0.89 ms; the
slowest warm call 2.49 ms (the one-pass hierarchy: nine ``do()`` and the round); two calls pay a
one-off cost of the process, 21.7 ms for the first ``FedAvg.do`` and 1,559 ms for the first fused
FedOPT round.  Every test runs its ``ready`` half first, so the ``late`` half never meets those
two; 20x the slowest warm call is 50 ms, 20x the cold FedAvg call 434 ms, 20x the cold FedOPT
round is far past the cap.  DELAY_MS = 150 ms: 60x the slowest warm call, and with up to three
delays per test it keeps every test under a second.  Should a call ever
outlast it, ``Late.call`` fails the test; it does not pass on luck.  The delay is calibrated once
per module with events around CAL_OPS adds; on that machine an add over 256 MiB took 0.0732 ms and
the delay came to CALIBRATED_OPS adds (for the record only: each session calibrates its own).
"""
import contextlib
import math
import time
from collections import OrderedDict

import torch

DEV = "cuda:0"
POISON = -7
DELAY_BYTES = 256 << 20
BALLAST_BYTES = 128 << 20
CAL_OPS = 16
# see "Delay length" above
ISSUE_MS_MEASURED = 2.49
DELAY_MS = 150.0
CALIBRATED_OPS = 2049

ISSUE_MS = []        # (label, ms) of every library call made in ``ready`` mode, in order


class Delay:
    """``DELAY_MS`` of ordinary torch work on the current stream; the buffer lives as long as this."""

    def __init__(self, ms=None):
        self.ms = DELAY_MS if ms is None else ms
        self._ballast = self._scalar = None
        self.buf = torch.zeros(DELAY_BYTES // 4, dtype=torch.float32, device=DEV)
        for _ in range(3):
            self.buf.add_(1.0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CAL_OPS):
            self.buf.add_(1.0)
        e1.record()
        e1.synchronize()
        self.ms_per_op = e0.elapsed_time(e1) / CAL_OPS
        self.ops = max(1, math.ceil(self.ms / self.ms_per_op))

    def enqueue(self):
        """The delay on the current stream and the event behind it."""
        self.buf.zero_()
        for _ in range(self.ops):
            self.buf.add_(1.0)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def ballast(self):
        """{a device scalar, BALLAST_BYTES of pinned host memory}: an update whose insert into a
        DeviceUpdateCache keeps the cache's side stream busy with one H2D copy for some milliseconds
        AFTER that stream has waited for the caller's (one key is device-resident).  The inserts
        queued behind it are then certainly later than the caller's next kernel -- unless that kernel
        waits for them, as it must."""
        if self._ballast is None:
            self._ballast = torch.zeros(BALLAST_BYTES // 4, dtype=torch.float32).pin_memory()
            self._scalar = torch.zeros(1, device=DEV)
        return OrderedDict([("dev", self._scalar), ("host", self._ballast)])

    def free(self):
        self.buf = self._ballast = self._scalar = None
        torch.cuda.empty_cache()


def poison_like(t, where="gpu"):
    if where == "gpu":
        return torch.full(tuple(t.shape), POISON, dtype=t.dtype, device=DEV)
    return torch.full(tuple(t.shape), POISON, dtype=t.dtype).pin_memory()


class Late:
    """One case's stream, poisoned buffers and reveals.  ``group``: which ``start`` reveals a buffer
    (a round number); every buffer of every group is poisoned before the one synchronise."""

    def __init__(self, delay, ready=False, stream=None):
        self.delay, self.ready = delay, ready
        self.s = None if ready else (stream or torch.cuda.Stream(DEV))
        self.groups = {}
        self.synced = False
        self.ev = None

    # ---- inputs
    def tensor(self, true, where="gpu", group=0):
        """``true`` (a CPU tensor) as the library will read it: on the device, or pinned; pageable
        host tensors (``where="host"``) cannot be written late and are simply copies."""
        if where == "host":
            return true.clone()
        if self.ready:
            return true.to(DEV, copy=True) if where == "gpu" else true.clone().pin_memory()
        assert not self.synced, "make every buffer before the first start()"
        with torch.cuda.stream(self.s):        # from s's pool, so reuse() gets the same blocks back
            buf = poison_like(true, where)
        self.groups.setdefault(group, []).append((buf, true.to(DEV)))
        return buf

    def weights(self, w, where="gpu", group=0):
        return OrderedDict((k, self.tensor(v, where, group)) for k, v in w.items())

    # ---- the stream
    def stream(self):
        if self.ready:
            return contextlib.nullcontext()
        if not self.synced:
            torch.cuda.synchronize()
            self.synced = True
        return torch.cuda.stream(self.s)

    def start(self, group=0):
        """Under ``stream()``: the delay, the event behind it, then the group's true values."""
        if self.ready:
            return
        assert torch.cuda.current_stream() == self.s
        self.ev = self.delay.enqueue()
        for buf, staged in self.groups.pop(group, ()):
            buf.copy_(staged, non_blocking=True)

    @contextlib.contextmanager
    def call(self, label, sync=None):
        """Around one library call.  Asynchronous by contract (``sync=None``): the delay must still be
        running when it returns.  ``sync``: the documented synchronisation that makes that impossible."""
        t0 = time.perf_counter()
        yield
        if self.ready:
            ISSUE_MS.append((label, (time.perf_counter() - t0) * 1e3))
        elif sync is None:
            assert self.ev is not None, "start() first"
            assert not self.ev.query(), (f"{label}: the delay ({self.delay.ms} ms, {self.delay.ops} ops) ran out "
                                         "before the call returned: nothing was late")
        else:
            assert isinstance(sync, str) and sync

    def reuse(self, *dicts):
        """Step 7 of the module docstring: ``dicts`` are emptied (the caller holds no other reference
        to their device tensors) and as many bytes are allocated and poisoned on the stream."""
        if self.ready:
            return
        specs = []
        for d in dicts:
            specs += [(tuple(v.shape), v.dtype) for v in d.values() if isinstance(v, torch.Tensor) and v.is_cuda]
            d.clear()
        self._refill = [torch.full(sh, POISON, dtype=dt, device=DEV) for sh, dt in specs]

    def snap(self, w):
        """A copy of a result taken on the current stream (ordered behind the library's work on it);
        a host tensor is read where it is, now."""
        return OrderedDict((k, w[k].detach().clone()) for k in w)

    def finish(self):
        if not self.ready:
            assert not self.groups, f"groups never revealed: {list(self.groups)}"
            self.s.synchronize()


def cpu(w):
    return OrderedDict((k, w[k].detach().cpu()) for k in w)


def assert_same(label, a, b):
    """Two runs' results (``{name: {key: tensor}}``) hold the same bits (a NaN equals a NaN)."""
    assert list(a) == list(b), label
    for name in a:
        assert list(a[name]) == list(b[name]), (label, name)
        for k in a[name]:
            x, y = a[name][k].detach().cpu(), b[name][k].detach().cpu()
            assert x.dtype == y.dtype and x.shape == y.shape, (label, name, k)
            xb, yb = x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)
            assert torch.equal(xb, yb), f"{label}: {name}/{k} differs between the default stream and the late one"
