"""Host side of the drop-in path: turns state_dict tensors into segment tables
and launches the native kernels (``include/flame_amd.h``) on torch's current stream.

Pure-Python planning (``plan``, ``plan_hier``, ``plan_feddyn``, ``rate32``,
``chunk_elems``) needs no GPU and is unit-tested on CPU; the launchers (``reduce_``,
``fedopt_reduce_adapt_``, ``fedopt_chain_``, ``scale_add_``, ``hier_fedbuff_``,
``feddyn_round_``, ``update_stats``, ``trimmed_mean``, ``noise_fill``, ``synth_fill_``) need the native
library and a HIP device.

Every launcher takes ONE path to the library: tensors grouped per dtype (``by_dtype``),
segments, a metadata block from one of the plan functions (all built on ``_Block``), then
``_launch``.  ``_launch`` alone decides whether the block rides in the kernel arguments or is
uploaded as a device table, runs the entry point under the timing hooks and checks its status;
the caller only says how each entry point is called.  What reaches the library this way is
pinned without a GPU by tests/test_engine_launch_trace.py.

A *segment* is one contiguous tensor (one state_dict entry).  For a reduction,
row ``s`` of the client table holds, in cache.iterkeys() order, the device
address of every client's tensor for segment ``s``.  One launch covers all
segments of one dtype, so a whole model aggregates in one kernel per dtype.
"""
from __future__ import annotations

import collections
import ctypes
import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import mx, shm_lease

DTYPE_CODE = {
    torch.float32: N.FLAME_F32, torch.bfloat16: N.FLAME_BF16, torch.float16: N.FLAME_F16,
    torch.float64: N.FLAME_F64, torch.int64: N.FLAME_I64, torch.int32: N.FLAME_I32,
}
FLOAT_CODES = (N.FLAME_F32, N.FLAME_BF16, N.FLAME_F16, N.FLAME_F64)
# state_dict dtypes the kernels do not carry (bool masks, uint8 / int8 / int16 buffers): their
# tmp is formed in fp32 by the kernel and cast, their adds are torch's (see tmp_of)
NARROW = (torch.bool, torch.uint8, torch.int8, torch.int16)
VEC_BYTES = 16
ITEMSIZE = {N.FLAME_F32: 4, N.FLAME_BF16: 2, N.FLAME_F16: 2, N.FLAME_F64: 8, N.FLAME_I64: 8, N.FLAME_I32: 4,
            N.FLAME_FP8_E4M3: 1, N.FLAME_FP8_E5M2: 1}
# update dtypes that one launch sums into an fp32 aggregate (flame_agg_reduce_mixed): a trainer's
# 16-bit deltas into the server's fp32 model.  Every other pair of differing dtypes stays on
# _accumulate_mixed / _accumulate_promoted.
UPLINK16 = (torch.bfloat16, torch.float16)
# element dtypes of an MX update (flame_amd.mx.MXWeights: float8 elements or packed float4 ones, one
# E8M0 scale byte per MX_BLOCK elements), which one flame_agg_reduce_mx / flame_agg_reduce_mxfp4 launch
# per format sums into an fp32 aggregate.  They are NOT in DTYPE_CODE (nor is the packed one in
# ITEMSIZE: half a byte): no other kernel, slab or cache takes them (:func:`mx_route`).
MX_PACKED = torch.float4_e2m1fn_x2      # two e2m1 elements per byte: a 1-D tensor of ceil(numel / 2) bytes
MX_CODE = {torch.float8_e4m3fn: N.FLAME_FP8_E4M3, torch.float8_e5m2: N.FLAME_FP8_E5M2, MX_PACKED: N.FLAME_FP4_E2M1}
MX_BLOCK = 32
MX_SUPPORTED = ("MX updates are supported as flame_amd.mx.MXWeights whose every entry holds the key in ONE float8 "
                "format (float8_e4m3fn or float8_e5m2), or packed as a 1-D float4_e2m1fn_x2 tensor of ceil(numel / 2) "
                "bytes with the aggregate's shape in MXWeights.shapes, with a 1-D uint8 scale tensor of ceil(numel / 32) "
                "bytes, summed "
                "into an fp32 aggregate by engine.accumulate / reduce_ (FedAvg, FedProx, FedGFT and the FedOPT family)")


def mx_row_len(dt, numel: int) -> int:
    """Elements of dtype ``dt`` an MX client tensor holds for ``numel`` logical elements (bytes, both ways)."""
    return -(-numel // 2) if dt == MX_PACKED else numel


def dtype_code(dt: torch.dtype) -> int:
    try:
        return DTYPE_CODE[dt]
    except KeyError:
        if dt in MX_CODE:
            raise TypeError(f"flame_amd: {dt} is the element dtype of an MX update, which only the reduction into an "
                            f"fp32 aggregate reads: the update guard, trim, krum, rfa, slabs and every other kernel "
                            f"do not take it.  {MX_SUPPORTED}") from None
        raise TypeError(f"flame_amd: tensor dtype {dt} is not supported by the aggregation kernels "
                        f"(supported: {sorted(str(d) for d in DTYPE_CODE)})") from None


_CHUNK = {}


def chunk_elems(code: int, scale_add: bool = False) -> int:
    """Elements one workgroup covers per chunk, as compiled into the library
    (flame_chunk_elems / flame_scale_add_chunk_elems; the library loads without a GPU)."""
    key = (code, scale_add)
    if key not in _CHUNK:
        L = N.lib()
        _CHUNK[key] = int(L.flame_scale_add_chunk_elems(code) if scale_add else L.flame_chunk_elems(code))
        if _CHUNK[key] <= 0:
            raise TypeError(f"flame_amd: dtype code {code} not supported by this kernel")
    return _CHUNK[key]


def rate32(rate: float) -> float:
    """torch wraps a Python float scalar and rounds it to the fp32 opmath type (RNE)."""
    return float(np.float32(rate))


# ------------------------------------------------------------------ planning (host only)
SEG_WORDS = 10  # int64 words per flame_segment


@dataclass
class Seg:
    numel: int
    out: int = 0
    inp: int = 0
    cur: int = 0
    cur_out: int = 0
    m: int = 0
    v: int = 0
    clients: List[int] = field(default_factory=list)
    tile_stride: int = 0   # bytes between consecutive chunks of one client (0 = contiguous)
    flags: int = 0         # FLAME_SEG_* bits set by the caller (FLAME_SEG_UNALIGNED is computed)
    bscales: Optional[List[int]] = None   # flame_agg_reduce_mx: one scale-byte pointer per client (any alignment)

    def pointers(self):
        return [self.out, self.inp, self.cur, self.cur_out, self.m, self.v, self.tile_stride] + list(self.clients)


@dataclass
class Plan:
    code: int
    meta: np.ndarray      # int64 words: [segments (10 each)] [client table] [rates32 | rates64]
    n_segs: int
    n_chunks: int
    n_clients: int
    off_clients: int      # byte offsets into the device copy of ``meta``
    off_r32: int
    off_r64: int
    off_s32: int = -1     # the per-client clip scales (flame_agg_reduce_scaled), -1 without them
    off_s64: int = -1
    off_bscales: int = -1  # the block-scale pointer table [n_segs][n_clients] (flame_agg_reduce_mx), -1 without it


class _Block:
    """A launch's metadata block under construction: the chunk cursor of its segments, the
    unaligned test of a segment's pointers, and the parts (arrays of 64-bit words, 32-bit arrays
    padded to 8 bytes) with the byte offset each one starts at."""

    def __init__(self, chunk: int):
        self.chunk, self.n_chunks = chunk, 0
        self.parts, self.offs, self.nbytes = [], {}, 0

    def chunk_begin(self, numel: int) -> int:
        """First chunk of a segment of ``numel`` elements; the cursor moves past it."""
        begin = self.n_chunks
        self.n_chunks += -(-numel // self.chunk) if numel > 0 else 0
        return begin

    @staticmethod
    def unaligned(fixed, *rows) -> int:
        """FLAME_SEG_UNALIGNED if a segment's fixed pointer or table row misses 16 bytes."""
        for r in rows:
            if (r % VEC_BYTES).any():
                return N.FLAME_SEG_UNALIGNED
        return N.FLAME_SEG_UNALIGNED if any(p % VEC_BYTES for p in fixed) else 0

    def add(self, name: str, a: np.ndarray) -> int:
        """Append a part; returns (and keeps under ``name``) its byte offset."""
        a = a.reshape(-1)
        if a.itemsize == 4 and a.size % 2:
            a = np.concatenate([a, np.zeros(1, a.dtype)])
        off = self.offs[name] = self.nbytes
        self.parts.append(a.view(np.int64))
        self.nbytes += a.nbytes
        return off

    def finish(self):
        """(int64 words of the block, chunks of the launch: all segments empty keeps one idle chunk)."""
        return np.concatenate(self.parts), max(self.n_chunks, 1)


def _f32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).reshape(-1).astype(np.float32)   # RNE, as torch rounds scalars


def plan(code: int, segs: Sequence[Seg], rates: Sequence, chunk: Optional[int] = None,
         seg_rates: bool = False, compact: bool = False, scales: Optional[Sequence] = None) -> Plan:
    """Build the device metadata block for one launch (no GPU needed).

    ``rates`` holds one rate per client, or with ``seg_rates`` one row of rates per
    segment (FLAME_AGG_SEG_RATES).  ``compact`` keeps only the rate array the dtype
    reads (its other offset is -1) -- the kernel-argument launch path.  ``scales`` (one
    per client, flame_agg_reduce_scaled) ride behind the rates, rounded as the rates are:
    fp32 RNE for f32 / bf16 / f16, the doubles themselves for f64."""
    n_segs = len(segs)
    if n_segs == 0:
        raise ValueError("empty segment list")
    if seg_rates:
        if len(rates) != n_segs or len({len(r) for r in rates}) > 1:
            raise ValueError("seg_rates: one equal-length rate row per segment")
        n = len(rates[0])
        rates = [r for row in rates for r in row]
    else:
        n = len(rates)
    b = _Block(chunk or chunk_elems(code))
    head = np.zeros((n_segs, SEG_WORDS), dtype=np.uint64)
    table = np.empty((n_segs, n), dtype=np.uint64)
    for i, s in enumerate(segs):
        if len(s.clients) != n:
            raise ValueError("every segment needs one pointer per client")
        table[i] = s.clients
        fixed = (s.out, s.inp, s.cur, s.cur_out, s.m, s.v)
        head[i] = (*fixed, s.numel, b.chunk_begin(s.numel), s.flags | b.unaligned(fixed, table[i]), s.tile_stride)
    b.add("segs", head)
    off_clients = b.add("clients", table)
    off_bscales = -1
    if any(s.bscales is not None for s in segs):
        if seg_rates or compact or any(s.bscales is None or len(s.bscales) != n for s in segs):
            raise ValueError("block scales: one pointer per client for every segment, device-table plans only")
        off_bscales = b.add("bscales", np.asarray([s.bscales for s in segs], dtype=np.uint64))
    r64 = np.asarray(rates, dtype=np.float64).reshape(-1)
    f64 = code == N.FLAME_F64       # compact: only the rate array the dtype reads (f64 tensors the fp64 rates)
    off_r32 = b.add("r32", _f32(r64)) if not (compact and f64) else -1
    off_r64 = b.add("r64", r64) if not compact or f64 else -1
    off_s32 = off_s64 = -1
    if scales is not None:
        if seg_rates or compact or len(scales) != n:
            raise ValueError("scales: one per client, device-table plans with one rate per client only")
        s64 = np.asarray(scales, dtype=np.float64).reshape(-1)
        off_s32 = b.add("s32", _f32(s64))
        off_s64 = b.add("s64", s64)
    meta, n_chunks = b.finish()
    return Plan(code, meta, n_segs, n_chunks, n, off_clients, off_r32, off_r64, off_s32, off_s64, off_bscales)


# ------------------------------------------------------------------ device staging
class _Staging:
    """Pinned host -> device upload of plan metadata, ordered on the current stream."""

    def __init__(self):
        self._inflight = collections.deque()
        self._streams = {}

    def upload(self, meta: np.ndarray, device: torch.device) -> torch.Tensor:
        """The copy runs on a side stream, so it overlaps whatever kernel the launch stream is
        still running (the next launch only waits for its own few-KB table, not for a copy
        queued behind the previous kernel); the launch stream waits on the copy's event."""
        while self._inflight and self._inflight[0][0].query():
            self._inflight.popleft()
        host = torch.from_numpy(meta)
        try:
            host = host.pin_memory()
        except RuntimeError:
            pass
        cur = current_stream(device)
        side = self._streams.get(device)
        if side is None:
            side = self._streams[device] = torch.cuda.Stream(device)
        with torch.cuda.stream(side):
            dev = host.to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        cur.wait_event(ev)
        dev.record_stream(cur)      # allocated on the side stream, read by kernels on the launch stream
        self._inflight.append((ev, host))
        return dev

    def drain(self) -> None:
        """Wait for every in-flight staging copy / zero-copy read and drop the host refs."""
        while self._inflight:
            ev, _ = self._inflight.popleft()
            ev.synchronize()

    def hold_on(self, stream, host_tensors) -> None:
        """Keep host tensors an asynchronous copy on ``stream`` reads alive until it has passed
        this point (a view of a sender's shared-memory segment: wait here, see ``hold``)."""
        ev = torch.cuda.Event()
        ev.record(stream)
        if any(shm_lease.aliases(t) for t in host_tensors):
            ev.synchronize()
            return
        self._inflight.append((ev, list(host_tensors)))

    def hold(self, host_tensor: torch.Tensor, device) -> None:
        """Keep a host tensor a kernel reads directly alive until the stream passes this point.
        A view into a sender's shared-memory segment is instead waited for here: the sender
        may rewrite the segment once the launching call has returned (shm_lease)."""
        ev = torch.cuda.Event()
        ev.record(current_stream(device))
        if shm_lease.aliases(host_tensor):
            ev.synchronize()
            return
        self._inflight.append((ev, host_tensor))


_staging = _Staging()

# Optional kernel timing hooks: when ``kernel_events`` is a list (bench.py), or while a
# flame_amd.metrics.KernelRecorder is active (``_recorders``), every native launch
# appends (name, start_event, end_event, algorithmic_bytes).  Events are recorded on
# the stream the kernel is launched on (torch's current stream).
kernel_events = None
_recorders = []


class _timed:
    def __init__(self, name, device, nbytes):
        self.name, self.device, self.nbytes = name, device, nbytes
        self.on = False

    def __enter__(self):
        self.on = kernel_events is not None or bool(_recorders)
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record(current_stream(self.device))
        return self

    def __exit__(self, *exc):
        if self.on and exc[0] is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(current_stream(self.device))
            ev = (self.name, self.e0, e1, self.nbytes)
            if kernel_events is not None:
                kernel_events.append(ev)
            for r in _recorders:
                r.append(ev)
        return False


def _dev_index(device) -> int:
    device = torch.device(device) if not isinstance(device, torch.device) else device
    return device.index if device.index is not None else torch.cuda.current_device()


def _stream_ptr(device) -> int:
    """The raw HIP stream torch's current stream is on ``device`` (no Stream object made)."""
    return torch._C._cuda_getCurrentRawStream(_dev_index(device))


_STREAMS = {}


def current_stream(device) -> torch.cuda.Stream:
    """``torch.cuda.current_stream(device)``, the Stream object kept per (device, raw stream):
    torch's own call builds a new one each time, several per launch on the small-round path.
    (torch's pooled streams are never destroyed, so a raw pointer names one stream for good.)"""
    idx = _dev_index(device)
    key = (idx, torch._C._cuda_getCurrentRawStream(idx))
    st = _STREAMS.get(key)
    if st is None:
        st = _STREAMS[key] = torch.cuda.current_stream(idx)
    return st


def _keepalive(tensors, device):
    """Call AFTER the launch: device tensors join the stream's allocator bookkeeping,
    zero-copy host tensors are held until an event recorded behind the kernel fires."""
    st = current_stream(device)
    for t in tensors:
        if t.is_cuda:
            t.record_stream(st)
        else:
            _staging.hold(t, device)


def _stage(meta: np.ndarray, device, keep) -> torch.Tensor:
    """The device copy of a metadata block, kept in ``keep`` (a caller that must stage every
    block before its first launch hands the copy to :func:`_launch` instead of the block)."""
    dm = _staging.upload(meta, device)
    keep.append(dm)
    return dm


def _launch(name, nbytes, device, keep, meta, table, argmeta=None) -> None:
    """THE path of every native launch: ``name`` and ``nbytes`` (algorithmic bytes) go to the
    timing hooks, the entry point's status to ``N.check``.

    ``meta`` is the launch's metadata block.  It rides in the kernel arguments --
    ``argmeta(host address, bytes)`` -- when ARGMETA is on, the caller offers that entry point and
    the block fits :func:`argmeta_max_bytes`; otherwise it is uploaded (the device copy joins
    ``keep``) and ``table(device base address)`` runs.  ``meta`` may be a copy :func:`_stage` made
    earlier, or None for a launch without a block (``table(None)``)."""
    if argmeta is not None and ARGMETA and meta.nbytes <= argmeta_max_bytes():
        with _timed(name, device, nbytes):
            N.check(argmeta(meta.ctypes.data, meta.nbytes))
        return
    if isinstance(meta, np.ndarray):
        meta = _stage(meta, device, keep)
    base = meta.data_ptr() if meta is not None else None
    with _timed(name, device, nbytes):
        N.check(table(base))


def by_dtype(items, dtype_of, also=None) -> "collections.OrderedDict":
    """``items`` grouped by the kernel dtype code of ``dtype_of(item)``: code -> items, codes and
    items in first-seen order (one launch per dtype).  With ``also`` the key is
    ``(code, also(item))``."""
    groups = collections.OrderedDict()
    for x in items:
        code = dtype_code(dtype_of(x))
        groups.setdefault(code if also is None else (code, also(x)), []).append(x)
    return groups


# ------------------------------------------------------------------ launches
# Zero-copy ingest: a pinned (hipHostMalloc'd) host tensor is device-addressable, so the
# kernel can stream client updates straight from host memory over PCIe instead of
# staging them into HBM first (FLAME_AMD_ZERO_COPY=0 disables).
ZERO_COPY_PINNED = os.environ.get("FLAME_AMD_ZERO_COPY", "1") != "0"


def _as_device(t: torch.Tensor, device) -> torch.Tensor:
    if t.device != device:
        if t.device.type == "cpu":
            shm_lease.check_live(t)     # a view of a sender's segment that has been rewritten raises
        if ZERO_COPY_PINNED and t.device.type == "cpu" and t.is_contiguous() and t.is_pinned():
            return t  # kept alive past the launch by _keepalive
        # a copy out of a sender's shared-memory segment completes before the call returns
        t = t.to(device, non_blocking=not shm_lease.aliases(t))
    return t.contiguous()


def _staged(t: torch.Tensor, device) -> torch.Tensor:
    """A contiguous device copy of ``t`` (``t`` itself when it already is one), never zero-copy:
    for optimizer state a kernel writes in place (FedOPT's ``m_t`` / ``v_t``) or whose address
    goes into a segment as it is (``current``, FedBuff's aggregate in :func:`scale_add_`).  The
    zero-copy branch of :func:`_as_device` is for read-only client rows, whose host addresses
    :func:`_client_row` translates."""
    if t.device != device:
        if t.device.type == "cpu":
            shm_lease.check_live(t)
        t = t.to(device, non_blocking=not shm_lease.aliases(t))
    return t.contiguous()


def tiled_stride(c: torch.Tensor, numel: int) -> int:
    """Bytes between chunks if ``c`` is a tiled slab view for a ``numel``-element
    aggregate (shape (ceil(numel/T), T), unit inner stride; see flame_amd/slab.py), else 0."""
    if c.dim() != 2 or not c.is_cuda or c.stride(1) != 1:
        return 0
    T = chunk_elems(dtype_code(c.dtype))
    if c.shape[1] != T or c.shape[0] != max(1, -(-numel // T)) or c.stride(0) < T:
        return 0
    return c.stride(0) * c.element_size()


def slice_elems(t: torch.Tensor, lo: int, hi: int, numel: int) -> torch.Tensor:
    """Elements [lo, hi) of a client tensor of ``numel`` logical elements, keeping a tiled
    slab view tiled (``lo`` must then be a multiple of the chunk)."""
    if t.is_cuda and tiled_stride(t, numel):
        T = t.shape[1]
        if lo % T:
            raise ValueError(f"tiled slice must start on a chunk boundary ({T})")
        return t[lo // T: -(-hi // T)]
    return t.reshape(-1)[lo:hi]


def uplink16_dtype(out_dtype, client_dtypes):
    """The clients' dtype where it differs from the aggregate's and one launch still takes them:
    an fp32 aggregate whose clients ALL hold bf16 or ALL hold f16 (:data:`UPLINK16`).  None for
    every other case, the same-dtype one included."""
    if out_dtype != torch.float32:
        return None
    it = iter(client_dtypes)
    first = next(it, None)
    if first not in UPLINK16 or any(dt != first for dt in it):
        return None
    return first


def is_mx(w) -> bool:
    """``w`` is an MX update, an :class:`flame_amd.mx.MXWeights`.  One isinstance, so the callers' hot
    paths pay nothing for asking; a float8 tensor in any other dict is refused where its dtype is
    looked at (:func:`dtype_code`, :func:`_check_cast`, :func:`reduce_`)."""
    return isinstance(w, mx.MXWeights)


def refuse_mx(ws, who: str) -> None:
    """TypeError when one of the updates ``ws`` is an MX update: ``who`` does not take them."""
    for w in ws:
        if w is not None and is_mx(w):
            raise TypeError(f"flame_amd: {who} does not take MX updates (a follow-up, not a silent slow path).  {MX_SUPPORTED}")


def mx_route(agg_dtype, ws, k, agg_shape=None):
    """The MX element dtype of key ``k`` when the updates ``ws`` (all carrying ``k``) take ONE
    flame_agg_reduce_mx / flame_agg_reduce_mxfp4 launch: every one an MXWeights holding ``k`` in the
    same element format with a 1-D uint8 scale tensor of ceil(numel / 32) bytes, under an fp32
    aggregate; a packed e2m1 key 1-D, of ceil(numel / 2) bytes, with its logical shape (``agg_shape``
    where the caller has it) in ``shapes``.  None when no update holds ``k`` as MX elements (its present
    route); every case in between is a TypeError."""
    dts = [weight_dtype(w, k) for w in ws]
    if not any(dt in MX_CODE for dt in dts):
        return None
    first = next(dt for dt in dts if dt in MX_CODE)
    if any(dt not in MX_CODE for dt in dts):
        other = next(dt for dt in dts if dt not in MX_CODE)
        raise TypeError(f"flame_amd: key {k!r} is {first} in some updates and {other} in others: per-key mixtures of MX "
                        f"and plain updates are not supported.  {MX_SUPPORTED}")
    if any(dt != first for dt in dts):
        raise TypeError(f"flame_amd: key {k!r} comes in two MX element formats ({first} and "
                        f"{next(dt for dt in dts if dt != first)}).  {MX_SUPPORTED}")
    if agg_dtype != torch.float32:
        raise TypeError(f"flame_amd: key {k!r}: MX updates into a {agg_dtype} aggregate are not supported.  {MX_SUPPORTED}")
    for w in ws:
        if not isinstance(w, mx.MXWeights):
            raise TypeError(f"flame_amd: key {k!r} is a {first} tensor in a plain {type(w).__name__}: a float8 tensor "
                            f"means nothing without its block scales.  {MX_SUPPORTED}")
        numel = w[k].numel()
        if first == MX_PACKED:
            shape = getattr(w, "shapes", {}).get(k)
            if shape is None:
                raise TypeError(f"flame_amd: key {k!r} is a {first} tensor without an MXWeights.shapes entry: two elements "
                                f"share a byte, so the packed tensor does not say how many it holds.  {MX_SUPPORTED}")
            numel = math.prod(shape)
            if w[k].dim() != 1:
                raise TypeError(f"flame_amd: key {k!r} is a {first} tensor of shape {tuple(w[k].shape)}, not 1-D.  {MX_SUPPORTED}")
            if w[k].numel() != -(-numel // 2):
                raise TypeError(f"flame_amd: key {k!r} is a {first} tensor of {w[k].numel()} bytes, not the {-(-numel // 2)} "
                                f"of its logical shape {tuple(shape)}.  {MX_SUPPORTED}")
            if agg_shape is not None and tuple(shape) != tuple(agg_shape):
                raise TypeError(f"flame_amd: key {k!r}: the MX update's logical shape {tuple(shape)} is not the aggregate's "
                                f"{tuple(agg_shape)}.  {MX_SUPPORTED}")
        s = w.scales.get(k)
        want = -(-numel // MX_BLOCK)
        if not isinstance(s, torch.Tensor):
            raise TypeError(f"flame_amd: key {k!r} is a {first} tensor without scales.  {MX_SUPPORTED}")
        if s.dtype != torch.uint8 or s.dim() != 1 or s.numel() != want:
            raise TypeError(f"flame_amd: key {k!r}: the MX scales are {s.dtype} {tuple(s.shape)}, not uint8 ({want},).  "
                            f"{MX_SUPPORTED}")
    return first


def _row_pointer(c: torch.Tensor, device, keep) -> int:
    """The device address the kernel reads a contiguous client tensor at: a device copy, or the
    translated address of a pinned host tensor (``keep``: what must outlive the launch)."""
    c = _as_device(c, device)
    keep.append(c)
    return c.data_ptr() if c.is_cuda else host_device_pointer(c.data_ptr())


def _client_row(cs, o: torch.Tensor, device, keep, cdt=None):
    """Device pointers of one segment's clients + the segment's client_tile_stride.

    If every client is a tiled slab view with the same stride, the kernel reads
    them tiled; otherwise every client is read contiguous (tiled views that are
    mixed with other layouts in one call are copied out -- rare).  ``cdt``: the clients' dtype
    where it is not the aggregate's (:func:`uplink16_dtype`); the tile-stride test is in it.  MX
    element tensors (``cdt`` a float8 dtype, or the packed float4 one: ceil(numel / 2) bytes) are never
    tiled: every row is contiguous."""
    n = o.numel()
    dt = cdt or o.dtype
    for c in cs:
        if c.dtype != dt:
            raise NotImplementedError(
                f"flame_amd: client tensor dtype {c.dtype} differs from aggregate dtype {dt}")
    if dt in MX_CODE:
        for c in cs:
            if c.numel() != mx_row_len(dt, n):
                raise RuntimeError(f"flame_amd: client tensor has {c.numel()} elements, aggregate {n}")
        # (a packed row is staged as its bytes: torch implements few operations on the float4 shell dtype)
        return [_row_pointer(c.view(torch.uint8) if dt == MX_PACKED else c, device, keep) for c in cs], 0
    if cs and cs[0].device == device:
        ts0 = tiled_stride(cs[0], n)
        if ts0:
            sh, st = cs[0].shape, cs[0].stride()
            if all(c.stride() == st and c.shape == sh and c.device == device for c in cs):
                if ts0 == chunk_elems(dtype_code(dt)) * ITEMSIZE[dtype_code(dt)]:
                    keep.extend(cs)   # ordinary contiguous (k, T) tensors: keep allocator bookkeeping
                # else: UpdateSlab views -- the slab outlives them, slot reuse is event-guarded
                return [c.data_ptr() for c in cs], ts0
    strides = [tiled_stride(c, n) if c.device == device else 0 for c in cs]
    row = []
    for c, ts in zip(cs, strides):
        if ts:
            c = c.reshape(-1)[:n]             # contiguous copy of a tiled view
        elif c.numel() != n:
            raise RuntimeError(f"flame_amd: client tensor has {c.numel()} elements, aggregate {n}")
        row.append(_row_pointer(c, device, keep))
    return row, 0


def _middle_rows(per_middle, o, device, keep):
    """One key's arrival pointers of a hierarchy, middle-major (``per_middle``: each middle's
    client tensors in arrival order; ``o`` as for :func:`_client_row`) with the one tile stride
    every middle's row has: ``(uint64 pointers, stride)``, or None when the strides differ."""
    ptrs, stride = [], None
    for cs in per_middle:
        row, ts = _client_row(cs, o, device, keep)
        if stride is None:
            stride = ts
        elif ts != stride:
            return None
        ptrs.extend(row)
    return np.asarray(ptrs, dtype=np.uint64), stride


def host_device_pointer(host_ptr: int) -> int:
    """Device address of a pinned / hipHostRegister-ed host address (zero-copy reads)."""
    out = ctypes.c_void_p()
    N.check(N.lib().flame_host_device_pointer(host_ptr, ctypes.byref(out)))
    return int(out.value or 0)


def _require_hip(device, who) -> None:
    if device.type != "cuda":
        raise RuntimeError(f"flame_amd.{who}: output tensors must live on the GPU (no CPU fallback)")


def reduce_(outs: List[torch.Tensor], ins: Optional[List[torch.Tensor]], clients: List[List[torch.Tensor]],
            rates: Optional[Sequence[float]], *, init_first: bool = False,
            seg_rates: Optional[Sequence[Sequence[float]]] = None,
            scales: Optional[Sequence[float]] = None,
            block_scales: Optional[Sequence[Optional[Sequence[torch.Tensor]]]] = None) -> None:
    """outs[s] = ins[s] (+)= Σ_i round(clients[s][i] * rates[i]) in order (kernel: flame_agg_reduce).

    ``outs`` are written in place (they must be contiguous device tensors);
    ``ins`` may be the same tensors (FedAvg mutates base_weights in place).
    ``seg_rates`` (instead of ``rates``) gives every segment its own rate row:
    independent reductions with equal client counts share one launch.
    ``scales`` (one per client; float dtypes, not with ``seg_rates``): each client's value is
    first multiplied by its clip scale, ``round(round(v * scale) * rate)`` (kernel:
    flame_agg_reduce_scaled).
    ``block_scales[s]`` (or None per segment): segment ``s``'s clients are MX element tensors
    (float8 or packed float4, :data:`MX_CODE`) and these are their uint8 E8M0 scale tensors, one per
    client; such segments under an fp32 output take one flame_agg_reduce_mx (float4:
    flame_agg_reduce_mxfp4) launch per element format, the clip ``scales`` inside it.
    """
    if not outs:
        return
    device = outs[0].device
    _require_hip(device, "reduce_")
    keep = []
    # a segment of 16-bit or MX clients under an fp32 output is grouped by both dtypes (ccode: the clients')
    cdts = [uplink16_dtype(o.dtype, (c.dtype for c in cs)) for o, cs in zip(outs, clients)]
    for s, (o, cs) in enumerate(zip(outs, clients)):
        mxs = block_scales[s] if block_scales is not None else None
        if mxs is None and any(c.dtype in MX_CODE for c in cs):
            raise TypeError(f"flame_amd.reduce_: float8 client tensors without block scales.  {MX_SUPPORTED}")
        if mxs is not None:
            cdts[s] = cs[0].dtype if cs else None
            if (cdts[s] not in MX_CODE or o.dtype != torch.float32 or len(mxs) != len(cs)
                    or any(c.dtype != cdts[s] for c in cs)
                    or (cdts[s] == MX_PACKED and any(c.dim() != 1 or c.numel() != -(-o.numel() // 2) for c in cs))
                    or any(m.dtype != torch.uint8 or m.dim() != 1 or m.numel() != -(-o.numel() // MX_BLOCK) for m in mxs)):
                raise TypeError(f"flame_amd.reduce_: segment {s} is not an MX segment.  {MX_SUPPORTED}")
    ccode_of = lambda dt: MX_CODE[dt] if dt in MX_CODE else dtype_code(dt)     # noqa: E731
    for (code, ccode), idx in by_dtype(range(len(outs)), lambda s: outs[s].dtype,
                                       also=lambda s: cdts[s] and ccode_of(cdts[s])).items():
        segs = []
        for s in idx:
            o = outs[s]
            assert o.is_contiguous() and o.device == device
            row, tstride = _client_row(clients[s], o, device, keep, cdts[s])
            brow = None
            if cdts[s] in MX_CODE:
                brow, _ = _client_row(block_scales[s], _KeyLike(-(-o.numel() // MX_BLOCK), torch.uint8), device, keep, torch.uint8)
            inp = 0
            if not init_first:
                i_t = ins[s]
                assert i_t.is_contiguous() and i_t.device == device and i_t.numel() == o.numel()
                inp = i_t.data_ptr()
            segs.append(Seg(o.numel(), out=o.data_ptr(), inp=inp, clients=row, tile_stride=tstride, bscales=brow))
        _launch_reduce(code, segs, rates if seg_rates is None else [seg_rates[s] for s in idx], device, keep,
                       init_first=init_first, seg_rates=seg_rates is not None, scales=scales, ccode=ccode)
    _keepalive(keep, device)


def _launch_reduce(code, segs, rates, device, keep, *, init_first=False, seg_rates=False, scales=None,
                   ccode=None) -> None:
    """One flame_agg_reduce launch over prepared segments (``keep`` holds what must outlive it);
    with ``scales`` one flame_agg_reduce_scaled launch (device tables only).  ``ccode``: the
    clients' dtype code where it differs from ``code`` -- one flame_agg_reduce_mixed launch
    (device tables only, chunks of the clients' dtype, ``scales`` inside the same entry point)."""
    L = N.lib()
    if ccode is not None and ccode != code:
        if init_first or seg_rates:
            raise NotImplementedError("flame_amd: 16-bit and MX updates into an fp32 aggregate take neither init_first "
                                      "(a None-start aggregate has the update's dtype) nor seg_rates")
        n_cl = _n_clients(rates, False)
        if ccode in MX_CODE.values():
            p = plan(ccode, segs, rates, scales=scales)
            flags = N.FLAME_AGG_XCD_MAP if p.n_chunks >= XCD_MAP_MIN_CHUNKS else 0
            if ccode == N.FLAME_FP4_E2M1:
                # per client ceil(numel / 2) bytes; per element one fp32 read and write; per block and client one scale byte
                nbytes = sum(n_cl * -(-s.numel // 2) + 2 * ITEMSIZE[code] * s.numel + n_cl * -(-s.numel // MX_BLOCK) for s in segs)
                _launch("flame_agg_reduce_mxfp4", nbytes, device, keep, p.meta,
                        lambda b: L.flame_agg_reduce_mxfp4(ccode, code, flags, b, p.n_segs, p.n_chunks, b + p.off_clients,
                                                           b + p.off_bscales, p.n_clients, b + p.off_r32,
                                                           b + p.off_s32 if scales is not None else None, _stream_ptr(device)))
                return
            # per element: n 1-byte reads, one fp32 read, one fp32 write; per block and client one scale byte
            nbytes = sum(s.numel * (n_cl + 2 * ITEMSIZE[code]) + n_cl * -(-s.numel // MX_BLOCK) for s in segs)
            _launch("flame_agg_reduce_mx", nbytes, device, keep, p.meta,
                    lambda b: L.flame_agg_reduce_mx(ccode, code, flags, b, p.n_segs, p.n_chunks, b + p.off_clients,
                                                    b + p.off_bscales, p.n_clients, b + p.off_r32,
                                                    b + p.off_s32 if scales is not None else None, _stream_ptr(device)))
            return
        nbytes = sum(s.numel for s in segs) * (n_cl * ITEMSIZE[ccode] + 2 * ITEMSIZE[code])
        p = plan(ccode, segs, rates, scales=scales)
        flags = N.FLAME_AGG_XCD_MAP if p.n_chunks >= XCD_MAP_MIN_CHUNKS and all(s.tile_stride == 0 for s in segs) else 0
        _launch("flame_agg_reduce_mixed", nbytes, device, keep, p.meta,
                lambda b: L.flame_agg_reduce_mixed(ccode, code, flags, b, p.n_segs, p.n_chunks, b + p.off_clients,
                                                   p.n_clients, b + p.off_r32,
                                                   b + p.off_s32 if scales is not None else None, _stream_ptr(device)))
        return
    flags = N.FLAME_AGG_INIT_FIRST if init_first else 0
    if seg_rates:
        flags |= N.FLAME_AGG_SEG_RATES
    n_cl = _n_clients(rates, seg_rates)
    nbytes = sum(s.numel for s in segs) * ITEMSIZE[code] * (n_cl + (1 if init_first else 2))
    if scales is not None and (seg_rates or code not in FLOAT_CODES):
        raise NotImplementedError("flame_amd: a scaled reduction takes float tensors and one rate per client")
    # the compact block's size is known before anything is built: a big launch builds one plan, not two
    est = compact_meta_bytes(code, len(segs), n_cl, seg_rates)
    if scales is None and ARGMETA and est <= argmeta_max_bytes():
        # small launch: the metadata block goes with the dispatch as a kernel argument (no H2D blit)
        p = plan(code, segs, rates, seg_rates=seg_rates, compact=True)
        assert p.meta.nbytes == est
        _launch("flame_agg_reduce", nbytes, device, keep, p.meta, None,
                lambda host, n: L.flame_agg_reduce_argmeta(code, flags, host, n, p.n_segs, p.n_chunks, p.n_clients,
                                                           p.off_clients, p.off_r32, p.off_r64, _stream_ptr(device)))
        return
    p = plan(code, segs, rates, seg_rates=seg_rates, scales=scales)
    if p.n_chunks >= XCD_MAP_MIN_CHUNKS and all(s.tile_stride == 0 for s in segs):
        # clients as separate tensors: each XCD streams a contiguous eighth of the chunks
        # (C3 rows 16.25 -> 15.89 ms; a tiled slab loses with it)
        flags |= N.FLAME_AGG_XCD_MAP
    if scales is None:
        _launch("flame_agg_reduce", nbytes, device, keep, p.meta,
                lambda b: L.flame_agg_reduce(code, flags, b, p.n_segs, p.n_chunks, b + p.off_clients, p.n_clients,
                                             b + p.off_r32, b + p.off_r64, _stream_ptr(device)))
    else:
        _launch("flame_agg_reduce_scaled", nbytes, device, keep, p.meta,
                lambda b: L.flame_agg_reduce_scaled(code, flags, b, p.n_segs, p.n_chunks, b + p.off_clients,
                                                    p.n_clients, b + p.off_r32, b + p.off_r64, b + p.off_s32,
                                                    b + p.off_s64, _stream_ptr(device)))


# Row-layout launches of at least this many chunks take the XCD-contiguous chunk map.
XCD_MAP_MIN_CHUNKS = int(os.environ.get("FLAME_AMD_XCD_MAP_MIN_CHUNKS", "4096"))

# Kernel-argument metadata for small launches (FLAME_AMD_ARGMETA=0 disables).
ARGMETA = os.environ.get("FLAME_AMD_ARGMETA", "1") != "0"
_ARGMETA_MAX = None


def argmeta_max_bytes() -> int:
    global _ARGMETA_MAX
    if _ARGMETA_MAX is None:
        _ARGMETA_MAX = int(N.lib().flame_agg_argmeta_max_bytes())
    return _ARGMETA_MAX


def compact_meta_bytes(code: int, n_segs: int, n_clients: int, seg_rates: bool = False) -> int:
    """Size of ``plan(..., compact=True)``'s block without building it: segments, client
    table and the one rate array the dtype reads (fp32 rates padded to 8 bytes)."""
    n_rates = (n_segs if seg_rates else 1) * n_clients
    return n_segs * (SEG_WORDS + n_clients) * 8 + (n_rates * 8 if code == N.FLAME_F64 else -(-n_rates // 2) * 8)


def _n_clients(rates, seg_rates) -> int:
    return len(rates[0]) if seg_rates else len(rates)


FEDOPT_VARIANT = {"fedadam": N.FLAME_FEDADAM, "fedyogi": N.FLAME_FEDYOGI, "fedadagrad": N.FLAME_FEDADAGRAD}


def fedopt_reduce_adapt_(variant: str, avg_out: List[Optional[torch.Tensor]], base: List[torch.Tensor],
                         cur: List[torch.Tensor], cur_out: List[torch.Tensor], m: List[torch.Tensor],
                         v: List[torch.Tensor], clients: List[List[torch.Tensor]], rates: Sequence[float],
                         hyper, state_zero: bool, cur_is_avg: Optional[Sequence[bool]] = None) -> None:
    """Fused FedAvg + FedOPT step (kernel: flame_fedopt_reduce_adapt, for fp64
    flame_fedopt_reduce_adapt_f64 with fp64 rates and ``hyper.raw``), one launch per dtype
    (fp32 / bf16 / fp16 / fp64; every tensor of a segment shares its dtype).  ``cur_is_avg[s]``:
    segment s's current weights ARE its FedAvg result (FLAME_SEG_CUR_IS_AVG: the caller's
    current aliases base, so d = avg - avg); ``cur[s]`` is then not read."""
    if not base:
        return
    device = base[0].device
    L = N.lib()
    groups = by_dtype(range(len(base)), lambda s: base[s].dtype)
    scalars = {code: _fedopt_group_scalars(code, hyper, base[idx[0]].dtype) for code, idx in groups.items()}
    aliased = cur_is_avg if cur_is_avg is not None else [False] * len(base)
    opt_flags = N.FLAME_OPT_STATE_ZERO if state_zero else 0
    for code, idx in groups.items():
        keep = []
        segs, p_alias = _fedopt_segs(idx, avg_out, base, cur, cur_out, m, v, clients, aliased, device, keep)
        nbytes = _fedopt_bytes(code, segs, len(rates), state_zero, p_alias)
        h = scalars[code]
        if code == N.FLAME_F64:
            # fp64 rates, the unrounded scalars, always the device table (no kernel-argument variant)
            p = plan(code, segs, rates)
            _launch("flame_fedopt_reduce_adapt", nbytes, device, keep, p.meta,
                    lambda b: L.flame_fedopt_reduce_adapt_f64(FEDOPT_VARIANT[variant], opt_flags, b, p.n_segs,
                                                              p.n_chunks, b + p.off_clients, p.n_clients,
                                                              b + p.off_r64, *h, _stream_ptr(device)))
        elif ARGMETA and compact_meta_bytes(code, len(segs), len(rates)) <= argmeta_max_bytes():
            # small round: the metadata block rides in the kernel arguments (no H2D blit)
            p = plan(code, segs, rates, compact=True)
            _launch("flame_fedopt_reduce_adapt", nbytes, device, keep, p.meta, None,
                    lambda host, n: L.flame_fedopt_reduce_adapt_argmeta(
                        code, FEDOPT_VARIANT[variant], opt_flags, host, n, p.n_segs, p.n_chunks, p.n_clients,
                        p.off_clients, p.off_r32, *h, _stream_ptr(device)))
        else:
            p = plan(code, segs, rates)
            _launch("flame_fedopt_reduce_adapt", nbytes, device, keep, p.meta,
                    lambda b: L.flame_fedopt_reduce_adapt(code, FEDOPT_VARIANT[variant], opt_flags, b, p.n_segs,
                                                          p.n_chunks, b + p.off_clients, p.n_clients, b + p.off_r32,
                                                          *h, _stream_ptr(device)))
        _keepalive(keep, device)


def _fedopt_segs(idx, outs, base, cur, cur_out, m, v, clients, aliased, device, keep):
    """Segments ``idx`` (one dtype group) of a FedOPT launch, and how many of their elements have
    no current to read.  ``outs[s]`` receives the FedAvg result (None: not written);
    ``aliased[s]``: segment s's current IS that result (FLAME_SEG_CUR_IS_AVG, ``cur[s]`` unread)."""
    segs, p_alias = [], 0
    for s in idx:
        b, alias = base[s], bool(aliased[s])
        for t in (b, cur_out[s], m[s], v[s]) + (() if alias else (cur[s],)):
            assert t.dtype == b.dtype and t.is_contiguous() and t.device == device
        row, tstride = _client_row(clients[s], b, device, keep)
        segs.append(Seg(b.numel(), out=outs[s].data_ptr() if outs[s] is not None else 0, inp=b.data_ptr(),
                        cur=0 if alias else cur[s].data_ptr(), cur_out=cur_out[s].data_ptr(), m=m[s].data_ptr(),
                        v=v[s].data_ptr(), clients=row, tile_stride=tstride,
                        flags=N.FLAME_SEG_CUR_IS_AVG if alias else 0))
        p_alias += b.numel() if alias else 0
    return segs, p_alias


def _fedopt_bytes(code, segs, n_clients, state_zero, p_alias) -> int:
    """clients + base + cur (+ m, v unless zero state) read once; avg / base, m, v, cur_out written once."""
    P = sum(sg.numel for sg in segs)
    return ITEMSIZE[code] * (P * (n_clients + 2 + (0 if state_zero else 2) + 4) - p_alias)


def _fedopt_group_scalars(code, hyper, dtype):
    """The six scalars a dtype group's kernel takes: the doubles for fp64, else the fp32 values."""
    if code == N.FLAME_F64:
        return _scalars64(hyper)
    h = [float(x) for x in hyper]
    if code in (N.FLAME_BF16, N.FLAME_F16):  # torch-CPU rounds the scalar of `sqrt(v) + tau`
        h[5] = float(torch.tensor(h[5], dtype=dtype))
    return h


def fedopt_chain_(variant: str, base: List[torch.Tensor], cur: List[Optional[torch.Tensor]],
                  cur_out: List[torch.Tensor], m: List[torch.Tensor], v: List[torch.Tensor],
                  clients: List[List[torch.Tensor]], rates: Sequence[float], step_end: Sequence[bool], hyper,
                  state_zero: bool, first_aliased: Sequence[bool]) -> None:
    """A queue of eager FedOPT do() calls in one pass (kernel: flame_fedopt_chain, for fp64
    flame_fedopt_chain_f64), one launch per dtype (fp32 / bf16 / fp16 / fp64; every tensor of a
    segment shares its dtype): per element,
    for each client in order, FedAvg into ``base`` (in place) with its rate, and after every
    client with ``step_end`` set, the adaptive step from the running current / m / v.
    ``first_aliased[s]``: segment s's current IS its base at the first step (``cur[s]`` unread);
    ``cur_out`` receives the final current, ``m`` / ``v`` are updated in place."""
    if not base:
        return
    device = base[0].device
    L = N.lib()
    if not step_end or not step_end[-1]:
        raise ValueError("fedopt_chain_: the last client must close a do() call")
    ends = np.zeros(-(-len(step_end) // 8) * 8, dtype=np.uint8)
    ends[:len(step_end)] = [1 if e else 0 for e in step_end]
    groups = by_dtype(range(len(base)), lambda s: base[s].dtype)
    for code, idx in groups.items():
        if code not in FLOAT_CODES:
            raise NotImplementedError(f"fedopt_chain_: dtype {base[idx[0]].dtype}")
    scalars = {code: _fedopt_group_scalars(code, hyper, base[idx[0]].dtype) for code, idx in groups.items()}
    opt_flags = N.FLAME_OPT_STATE_ZERO if state_zero else 0
    # every dtype group is planned and its tables uploaded BEFORE the first launch: a failure
    # there (a bad tensor, an allocation) leaves base / m / v untouched.  Only a
    # launch itself failing after another group's launch ran can leave the groups out of step;
    # that exception carries flame_partial = True (FedOPT then refuses further calls).
    launches = []
    for code, idx in groups.items():
        keep = []
        segs, p_alias = _fedopt_segs(idx, base, base, cur, cur_out, m, v, clients, first_aliased, device, keep)
        p = plan(code, segs, rates)
        # the step_end bytes ride behind the plan's tables: one upload per launch
        dm = _stage(np.concatenate([p.meta, ends.view(np.int64)]), device, keep)
        launches.append((code, p, dm, _fedopt_bytes(code, segs, len(rates), state_zero, p_alias), keep))
    for i, (code, p, dm, nbytes, keep) in enumerate(launches):
        h = scalars[code]
        if code == N.FLAME_F64:      # fp64 rates, the unrounded scalars
            def call(b):
                return L.flame_fedopt_chain_f64(FEDOPT_VARIANT[variant], opt_flags, b, p.n_segs, p.n_chunks,
                                                b + p.off_clients, p.n_clients, b + p.off_r64, b + p.meta.nbytes,
                                                *h, _stream_ptr(device))
        else:
            def call(b):
                return L.flame_fedopt_chain(code, FEDOPT_VARIANT[variant], opt_flags, b, p.n_segs, p.n_chunks,
                                            b + p.off_clients, p.n_clients, b + p.off_r32, b + p.meta.nbytes,
                                            *h, _stream_ptr(device))
        try:
            _launch("flame_fedopt_chain", nbytes, device, keep, dm, call)
        except Exception as e:
            if i:
                e.flame_partial = True
            raise
        _keepalive(keep, device)


class FedoptScalars(tuple):
    """The six fp32 scalars (a plain tuple to every caller that unpacks them), with the Python
    floats they were rounded from in ``raw``: an fp64 tensor multiplies by those unrounded."""

    def __new__(cls, rounded, raw):
        self = super().__new__(cls, rounded)
        self.raw = tuple(float(x) for x in raw)
        return self

    def __reduce__(self):
        return (FedoptScalars, (tuple(self), self.raw))


def fedopt_scalars(beta_1, beta_2, eta, tau):
    """fp32 scalars torch uses for `beta_1 * m`, `(1 - beta_1) * d`, ... (fedopt.py:113-129);
    ``.raw`` keeps the Python floats, which are what an fp64 tensor is multiplied by."""
    f = np.float32
    raw = (beta_1, 1 - beta_1, beta_2, 1 - beta_2, eta, tau)
    return FedoptScalars([f(x) for x in raw], raw)


def _scalars64(hyper):
    """The double scalars of an fp64 dtype group."""
    raw = getattr(hyper, "raw", None)
    if raw is None:
        raise TypeError("flame_amd: an fp64 FedOPT launch needs the unrounded scalars "
                        "(pass engine.fedopt_scalars(...), not its fp32 values)")
    return [float(x) for x in raw]


def scale_add_(bases: List[torch.Tensor], aggs: List[torch.Tensor], goal: int,
               deltas: Optional[List[torch.Tensor]] = None) -> None:
    """bases[s] += aggs[s] / goal in place; optional deltas[s] = new - old (flame_fedbuff_scale_add)."""
    if not bases:
        return
    device = bases[0].device
    L = N.lib()
    for b in bases:
        if not b.is_floating_point() or dtype_code(b.dtype) not in FLOAT_CODES:
            # torch: int_tensor / int -> float; in-place add into an int tensor raises
            raise RuntimeError(f"result type Float can't be cast to the desired output type "
                               f"{str(b.dtype).replace('torch.', '').capitalize()}")
    keep = []
    for code, idx in by_dtype(range(len(bases)), lambda s: bases[s].dtype).items():
        segs = []
        for s in idx:
            b = bases[s]
            # staged, not zero-copy: a.data_ptr() goes into the segment as it is, and the aggregate
            # is optimizer state (one H2D copy of a host-resident one), not a client row
            a = _staged(aggs[s], device)
            if a.numel() != b.numel():
                raise RuntimeError(f"flame_amd: scale_add of {a.numel()} elements into {b.numel()}")
            if a.dtype != b.dtype:
                _scale_add_promoted(b, a, goal, deltas[s] if deltas is not None else None, device)
                continue
            keep.append(a)
            d = deltas[s].data_ptr() if deltas is not None else 0
            segs.append(Seg(b.numel(), out=b.data_ptr(), inp=a.data_ptr(), cur_out=d))
        if not segs:
            continue
        p = plan(code, segs, [], chunk=chunk_elems(code, scale_add=True))
        nbytes = sum(s.numel for s in segs) * ITEMSIZE[code] * (3 + (1 if deltas is not None else 0))
        _launch("flame_fedbuff_scale_add", nbytes, device, keep, p.meta,
                lambda b: L.flame_fedbuff_scale_add(code, b, p.n_segs, p.n_chunks, int(goal), _stream_ptr(device)))
    _keepalive(keep, device)


def _scale_add_promoted(b: torch.Tensor, a: torch.Tensor, goal: int, delta, device) -> None:
    """``b += a / goal`` (fedbuff.py:126) when the aggregate's dtype is not the model's:
    ``q = a / goal`` is true division in a's dtype (int64 / int -> float32, torch's default
    dtype), formed by the scale_add kernel into a -0.0-filled buffer (x + -0 == x for every
    x, so the buffer holds exactly ``fl(a / goal)``); then the promoted in-place add
    (:func:`_add_promoted`); ``delta = new - old`` in b's dtype (common/util.py:152-159)."""
    af = a.reshape(-1)
    if not af.is_floating_point():
        af = af.to(torch.get_default_dtype())
    q = torch.full(af.shape, -0.0, dtype=af.dtype, device=device)
    scale_add_([q], [af], goal)
    old = b.clone() if delta is not None else None
    _add_promoted(b.view(-1), q)
    if delta is not None:
        from . import elementwise as ew
        dv = delta.view(-1)
        d = ew.Lazy.of(b.view(-1)) - ew.Lazy.of(old.view(-1))
        if d.dtype != dv.dtype:             # torch.sub(..., out=delta) casts into delta's dtype
            d = d.to(dv.dtype)
        if dv.is_cuda and dv.is_contiguous():
            ew.materialize(d, device=dv.device, into=[dv])
        else:
            dv.copy_(ew.materialize(d, device=device)[0])


# ------------------------------------------------------------------ co-located FedBuff hierarchy
HSEG_WORDS = N.HIER_SEGMENT_INT64S


@dataclass
class HierSeg:
    """One tensor of the hierarchy: the top's pointers + per-middle weight / delta pointers
    and the [n_mids * n_clients] arrival pointers (middle-major, arrival order)."""
    numel: int
    mid_w: Sequence[int]
    clients: Sequence[int]
    mid_delta: Optional[Sequence[int]] = None
    top_w: int = 0
    top_in: int = 0
    top_out: int = 0
    tile_stride: int = 0
    mid_tile_stride: int = 0   # bytes between chunks of one middle's weights (0 = contiguous)


@dataclass
class HierPlan:
    code: int
    meta: np.ndarray
    n_segs: int
    n_chunks: int
    n_mids: int
    n_clients: int
    offs: dict            # byte offsets of the tables inside the device copy of ``meta``


def plan_hier(code: int, segs: Sequence[HierSeg], mid_rates, mid_goals, top_rates) -> HierPlan:
    """Device metadata of one flame_hier_fedbuff launch (no GPU needed):
    [segments (8 words)] [mid_w S x M] [mid_delta S x M] [clients S x M x C]
    [mid_rates f32 M x C] [mid_goal f32 M] [top_rates f32 M]."""
    S = len(segs)
    if S == 0:
        raise ValueError("empty segment list")
    M = len(mid_goals)
    if M == 0 or len(top_rates) != M or len(mid_rates) != M:
        raise ValueError("one goal, one top rate and one rate row per middle")
    C = len(mid_rates[0])
    if C == 0 or any(len(r) != C for r in mid_rates):
        raise ValueError("every middle needs the same (>= 1) number of arrivals")
    b = _Block(chunk_elems(code))
    head = np.zeros((S, HSEG_WORDS), dtype=np.uint64)
    wtab = np.empty((S, M), dtype=np.uint64)
    dtab = np.zeros((S, M), dtype=np.uint64)
    ctab = np.empty((S, M * C), dtype=np.uint64)
    for i, s in enumerate(segs):
        if len(s.mid_w) != M or len(s.clients) != M * C or (s.mid_delta is not None and len(s.mid_delta) != M):
            raise ValueError("segment tables must be [n_mids] and [n_mids * n_clients]")
        wtab[i] = s.mid_w
        ctab[i] = s.clients
        if s.mid_delta is not None:
            dtab[i] = s.mid_delta
        fixed = (s.top_w, s.top_in, s.top_out)
        head[i] = (*fixed, s.numel, b.chunk_begin(s.numel), b.unaligned(fixed, ctab[i], wtab[i], dtab[i]),
                   s.tile_stride, s.mid_tile_stride)
    for nm, a in (("segs", head), ("mid_w", wtab), ("mid_delta", dtab), ("clients", ctab),
                  ("mid_rates", _f32(mid_rates)), ("mid_goal", _f32(mid_goals)), ("top_rates", _f32(top_rates))):
        b.add(nm, a)
    meta, n_chunks = b.finish()
    return HierPlan(code, meta, S, n_chunks, M, C, b.offs)


def hier_fedbuff_(segs: Sequence[HierSeg], code: int, mid_rates, mid_goals, top_rates, *, top_accum: bool,
                  top_goal: Optional[int], device, keep: list, mid_readonly: bool = False, sync: bool = False) -> None:
    """One flame_hier_fedbuff launch (the caller checked dtypes / devices / contiguity).
    ``sync``: the synchronous FedAvg hierarchy (FLAME_HIER_SYNC; needs ``top_accum``)."""
    L = N.lib()
    p = plan_hier(code, segs, mid_rates, mid_goals, top_rates)
    flags = ((N.FLAME_HIER_TOP_ACCUM if top_accum else 0) | (N.FLAME_HIER_TOP_APPLY if top_goal is not None else 0)
             | (N.FLAME_HIER_MID_READONLY if mid_readonly else 0) | (N.FLAME_HIER_SYNC if sync else 0))
    with_delta = any(s.mid_delta is not None for s in segs)
    P = sum(s.numel for s in segs)
    isz = ITEMSIZE[code]
    M, C = p.n_mids, p.n_clients
    # arrivals + middle weights (read, write) [+ deltas] + top (in) + top out [+ top weights r/w]
    # distinct middle-weight tensors (read-only middles may share one base: it is read once)
    wsum = sum(s.numel * len(set(int(p) for p in s.mid_w)) for s in segs)
    top_out = any(s.top_out for s in segs)
    nbytes = isz * (P * (M * C + (M if with_delta else 0) + (1 if top_accum else 0) + (1 if top_out else 0)
                         + (2 if top_goal is not None else 0)) + wsum * (1 if mid_readonly else 2))
    o = p.offs
    # a small launch (e.g. one FedBuff aggregator's fused scale_add) takes its metadata as a kernel argument
    _launch("flame_hier_fedbuff", nbytes, device, keep, p.meta,
            lambda b: L.flame_hier_fedbuff(code, flags, b + o["segs"], p.n_segs, p.n_chunks, M, C, b + o["mid_w"],
                                           b + o["mid_delta"] if with_delta else None, b + o["clients"],
                                           b + o["mid_rates"], b + o["mid_goal"], b + o["top_rates"],
                                           float(top_goal or 0), _stream_ptr(device)),
            lambda host, n: L.flame_hier_fedbuff_argmeta(code, flags, host, n, p.n_segs, p.n_chunks, M, C, o["mid_w"],
                                                         o["mid_delta"] if with_delta else -1, o["clients"],
                                                         o["mid_rates"], o["mid_goal"], o["top_rates"],
                                                         float(top_goal or 0), _stream_ptr(device)))


def hier_resident_per_cu(code: int, n_mids: int, sync: bool = False) -> int:
    """Resident workgroups per CU of the flame_hier_fedbuff launch for these arguments."""
    r = int(N.lib().flame_hier_resident_per_cu(code, N.FLAME_HIER_SYNC if sync else 0, int(n_mids)))
    if r < 1:
        N.check(-r)
    return r


# ------------------------------------------------------------------ FedDyn server round
def feddyn_program(arrivals: Sequence, dict_order: Sequence, had_history) -> tuple:
    """Step program of one flame_feddyn_round launch (host only, no GPU).

    ``arrivals``: the ends in cache.iterkeys() order; ``dict_order``: local_param_dict's
    order after this round's untracked ends were appended (feddyn.py:125-139);
    ``had_history``: ends whose history existed (not None) before the round.  Returns
    ``([(flags, end), ...], n_phase1)``.  The FedAvg sum must run in arrival order and the
    history mean in dict order (feddyn.py:96-112).  When the arrivals appear in dict
    order in the same relative order, both sums ride one merged step list (each update
    and history read once); otherwise phase 1 walks the arrivals (average + history
    update) and phase 2 re-reads the histories in dict order for the mean."""
    arrived = set(arrivals)
    pos = {e: i for i, e in enumerate(dict_order)}
    ap = [pos[e] for e in arrivals]
    merged = all(a < b for a, b in zip(ap, ap[1:]))
    hist = [e for e in dict_order if e in arrived or e in had_history]

    def arrival(e):
        return N.FLAME_DYN_W | N.FLAME_DYN_AVG | N.FLAME_DYN_HOUT | (N.FLAME_DYN_HIN if e in had_history else 0)

    if merged:
        steps = [((arrival(e) | N.FLAME_DYN_MEAN) if e in arrived else (N.FLAME_DYN_HIN | N.FLAME_DYN_MEAN), e)
                 for e in hist]
        return steps, len(steps)
    steps = [(arrival(e), e) for e in arrivals] + [(N.FLAME_DYN_HIN | N.FLAME_DYN_MEAN, e) for e in hist]
    return steps, len(arrivals)


@dataclass
class DynSeg:
    """One tensor of a FedDyn round: base / average / cld pointers and, per program step,
    (w, h_in, h_out) pointers (0 where the step has none)."""
    numel: int
    out: int
    inp: int
    cld: int
    steps: Sequence[Sequence[int]]
    tile_stride: int = 0
    hist_tile_stride: int = 0


def plan_feddyn(code: int, segs: Sequence[DynSeg], flags: Sequence[int]):
    """[segments (8 words)] [steps S x K x 3] [flags u32 K] -> (meta, n_chunks, byte offsets)."""
    S, K = len(segs), len(flags)
    if S == 0 or K == 0:
        raise ValueError("feddyn plan needs >= 1 segment and >= 1 step")
    b = _Block(chunk_elems(code))
    head = np.zeros((S, N.DYN_SEGMENT_INT64S), dtype=np.uint64)
    tab = np.zeros((S, K * 3), dtype=np.uint64)
    for i, s in enumerate(segs):
        if len(s.steps) != K:
            raise ValueError("every segment needs one pointer triple per step")
        tab[i] = np.asarray(s.steps, dtype=np.uint64).reshape(-1)
        fixed = (s.out, s.inp, s.cld)
        head[i] = (*fixed, s.numel, b.chunk_begin(s.numel), b.unaligned(fixed, tab[i]), s.tile_stride,
                   s.hist_tile_stride)
    b.add("segs", head)
    b.add("steps", tab)
    b.add("flags", np.asarray(flags, dtype=np.uint32))
    meta, n_chunks = b.finish()
    return meta, n_chunks, b.offs


def feddyn_round_(code: int, segs: Sequence[DynSeg], flags: Sequence[int], n_phase1: int, rate_avg: float,
                  rate_mean: float, device, keep: list) -> None:
    """One flame_feddyn_round launch (the caller checked dtypes / devices / contiguity)."""
    meta, n_chunks, offs = plan_feddyn(code, segs, flags)
    P = sum(s.numel for s in segs)
    reads = sum(bool(f & N.FLAME_DYN_W) + bool(f & N.FLAME_DYN_HIN) for f in flags)
    writes = sum(bool(f & N.FLAME_DYN_HOUT) for f in flags)
    nbytes = ITEMSIZE[code] * P * (reads + writes + 3)     # + base read, average and cld written
    _launch("flame_feddyn_round", nbytes, device, keep, meta,
            lambda b: N.lib().flame_feddyn_round(code, b + offs["segs"], len(segs), n_chunks, b + offs["steps"],
                                                 b + offs["flags"], len(flags), n_phase1, float(rate_avg),
                                                 float(rate_mean), _stream_ptr(device)))


def synth_fill_(out: torch.Tensor, seed: int, stream_id: int, start: int, sigma: float) -> None:
    """Fill a device tensor with flame_amd.synth values (bench / test inputs)."""
    from .synth import scale_for_sigma
    assert out.is_cuda and out.is_contiguous()
    N.check(N.lib().flame_synth_fill(dtype_code(out.dtype), out.data_ptr(), out.numel(), seed, stream_id,
                                     start, float(scale_for_sigma(sigma)), _stream_ptr(out.device)))


# ------------------------------------------------------------------ server-side Gaussian noise
def plan_noise(code: int, segs: Sequence[Seg], streams: Sequence[int], starts: Sequence[int],
               chunk: Optional[int] = None):
    """[segments (10 words)] [streams u32 S] [starts i64 S] -> (meta, n_chunks, byte offsets): the
    metadata block of one flame_noise_fill launch (no GPU needed).  The two arrays live in device
    memory, where the library cannot look before it launches: a negative start or a stream outside
    32 bits is refused here."""
    S = len(segs)
    if S == 0:
        raise ValueError("empty segment list")
    if len(streams) != S or len(starts) != S:
        raise ValueError("noise: one stream and one start per segment")
    for st in streams:
        if isinstance(st, bool) or not isinstance(st, (int, np.integer)) or not 0 <= int(st) < 1 << 32:
            raise ValueError(f"noise: a stream is the key's position in the model, an int in [0, 2^32), not {st!r}")
    for st in starts:
        if isinstance(st, bool) or not isinstance(st, (int, np.integer)) or not 0 <= int(st) < 1 << 62:
            raise ValueError(f"noise: a start is an element index >= 0 (below 2^62), not {st!r}")
    b = _Block(chunk or chunk_elems(code))
    head = np.zeros((S, SEG_WORDS), dtype=np.uint64)
    for i, s in enumerate(segs):
        head[i, 0] = s.out
        head[i, 6:9] = (s.numel, b.chunk_begin(s.numel), b.unaligned((s.out,)))
    b.add("segs", head)
    b.add("streams", np.asarray([int(x) for x in streams], dtype=np.uint32))
    b.add("starts", np.asarray([int(x) for x in starts], dtype=np.int64))
    meta, n_chunks = b.finish()
    return meta, n_chunks, b.offs


def check_noise_args(seed, rnd, std):
    """``(seed, round mod 2^32, std)`` as flame_noise_fill takes them; a bad value raises before any launch."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"noise: seed must be an int in [0, 2^64), not {seed!r}")
    if isinstance(rnd, bool) or not isinstance(rnd, (int, np.integer)) or int(rnd) < 0:
        raise ValueError(f"noise: round must be an int >= 0, not {rnd!r}")
    std = float(std)
    if not (std >= 0.0) or math.isinf(std):
        raise ValueError(f"noise: std must be a finite number >= 0, not {std!r}")
    return int(seed), int(rnd) & 0xFFFFFFFF, std


def noise_fill_(outs: List[torch.Tensor], streams: Sequence[int], starts: Sequence[int], seed: int, rnd: int,
                std: float) -> None:
    """outs[s][e] = round_dtype(z(seed, rnd, streams[s], starts[s] + e) * std), written in place
    (kernel: flame_noise_fill; Philox4x32-10 + Box-Muller, DESIGN.md §2 "the noise contract").  ``outs``
    are contiguous device tensors of f32 / bf16 / f16 / f64 (a view one element off alignment is
    written element by element); one launch per dtype on torch's current stream."""
    if not outs:
        return
    seed, rnd, std = check_noise_args(seed, rnd, std)
    device = outs[0].device
    if device.type != "cuda":
        raise RuntimeError("flame_amd.noise_fill_: output tensors must live on the GPU (no CPU fallback)")
    L = N.lib()
    keep = []
    for code, idx in by_dtype(range(len(outs)), lambda s: outs[s].dtype).items():
        if code not in FLOAT_CODES:
            raise TypeError(f"flame_amd.noise_fill_: {outs[idx[0]].dtype} tensors get no noise (float dtypes only)")
        for s in idx:
            assert outs[s].is_contiguous() and outs[s].device == device
        segs = [Seg(outs[s].numel(), out=outs[s].data_ptr() if outs[s].numel() else 0) for s in idx]
        meta, n_chunks, offs = plan_noise(code, segs, [streams[s] for s in idx], [starts[s] for s in idx])
        _launch("flame_noise_fill", sum(sg.numel for sg in segs) * ITEMSIZE[code], device, keep, meta,
                lambda b: L.flame_noise_fill(code, b + offs["segs"], len(segs), n_chunks, b + offs["streams"],
                                             b + offs["starts"], seed, rnd, std, _stream_ptr(device)))
    _keepalive(keep + list(outs), device)


def noise_fill(like: dict, seed: int, rnd: int, std: float, *, device=None) -> dict:
    """``{key: noise}`` for the FLOAT keys of ``like`` (a model's state_dict): new device tensors of each
    key's dtype and shape, ``noise[e] = round_dtype(z[e] * std)`` with ``z`` the fp32 unit normal of
    ``(seed, rnd, stream, e)`` and ``stream`` the key's position in ``like``'s iteration order, counting
    every key.  Integer and bool keys get no noise and are absent.  One flame_noise_fill launch per
    dtype on torch's current stream; nothing is read back."""
    seed, rnd, std = check_noise_args(seed, rnd, std)
    device = _hip_device(device, "noise_fill", prefer=like)
    keys, outs, streams = [], [], []
    for pos, (k, t) in enumerate(like.items()):
        if isinstance(t, torch.Tensor) and t.is_floating_point():
            dtype_code(t.dtype)                 # an unsupported float dtype raises
            keys.append(k)
            outs.append(torch.empty(t.shape, dtype=t.dtype, device=device))
            streams.append(pos)
    noise_fill_(outs, streams, [0] * len(outs), seed, rnd, std)
    return collections.OrderedDict(zip(keys, outs))


# ------------------------------------------------------------------ dict-level helpers used by the optimizers
def pick_device(*dicts) -> torch.device:
    for d in dicts:
        if d:
            for t in d.values():
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("flame_amd: no HIP device available; the MI355X aggregation path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _cuda_device_of(d):
    """The device of the first GPU tensor in dict ``d`` (None: it holds none)."""
    return next((t.device for t in d.values() if isinstance(t, torch.Tensor) and t.is_cuda), None)


def _hip_device(device, who, *dicts, prefer=None) -> torch.device:
    """Launcher ``who``'s device: ``device`` if given, else where ``prefer`` (the aggregate) lives, else
    :func:`pick_device` over ``dicts``; anything but a GPU raises, one without an index is the current."""
    if device is not None:
        device = torch.device(device)
    else:
        device = (prefer is not None and _cuda_device_of(prefer)) or pick_device(*dicts)
    if device.type != "cuda":
        raise RuntimeError(f"flame_amd.{who}: needs a HIP device (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _Target:
    """A tensor to be updated in place on the device; stages CPU / strided tensors."""

    def __init__(self, t: torch.Tensor, device):
        self.orig = t
        self.dev = t if (t.device == device and t.is_contiguous()) else t.to(device).contiguous()

    def writeback(self):
        if self.dev is not self.orig:
            self.orig.copy_(self.dev)


def accumulate(agg: dict, entries, *, device=None, key_groups=None, after_group=None, scales=None) -> None:
    """agg[k] += round(v_i[k] * rate_i) for entries (weights, rate) in order, in place.

    ``scales`` (one per entry, the update guard's clip scales): every FLOAT update tensor is
    first multiplied by its entry's scale, ``round(v * scale)`` in v's dtype
    (differential_privacy.py:79-82) -- same-dtype float keys inside the reduction
    (flame_agg_reduce_scaled), float tensors on the mixed / promoted path pre-scaled per entry
    with :func:`tmp_of`; integer and bool tensors are never scaled.

    Restates the per-client / per-key loop of fedavg.py:79-104 and fedbuff.py:89-97,
    136-157 (agg not None) as one launch per dtype over all keys and clients.

    ``key_groups`` (a partition of agg's keys, e.g. a parameter-sharded plan's waves):
    one launch per dtype per group, in group order, calling ``after_group(i)`` as soon
    as group ``i``'s launches are queued (the sharded path starts that group's
    all-gather there).  Pointer rows are still built once for all keys.
    """
    if not entries:
        return
    if device is None:   # the aggregate's own device first (no per-entry list for the common case)
        device = _cuda_device_of(agg) or pick_device(*[w for w, _ in entries])
    if scales is not None and len(scales) != len(entries):
        raise ValueError("accumulate: one scale per entry")
    if _accumulate_slab(agg, entries, device, key_groups, after_group, scales):
        return
    if key_groups is not None:
        refuse_mx([w for w, _ in entries], "the sharded wrapper (key_groups)")
        for w, _ in entries:
            for k in w.keys():
                if k not in agg:
                    raise KeyError(k)
        for gi, g in enumerate(key_groups):
            accumulate({k: agg[k] for k in g}, [({k: w[k] for k in g if k in w}, r) for w, r in entries],
                       device=device, scales=scales)
            if after_group is not None:
                after_group(gi)
        return
    keys = list(agg.keys())
    per_key = collections.OrderedDict()
    for ci, (w, _) in enumerate(entries):
        for k in w.keys():
            if k not in agg:
                raise KeyError(k)
            per_key.setdefault(k, []).append(ci)
    # group keys by participating-client set (normally every key has every client)
    groups = collections.OrderedDict()
    for k in keys:
        if k in per_key:
            groups.setdefault(tuple(per_key[k]), []).append(k)
    any_mx = any(is_mx(w) for w, _ in entries)      # (a float8 tensor in a plain dict: _check_cast refuses it)
    routed = []
    for cis, ks in groups.items():
        # MX keys: float8 elements + block scales of MXWeights under an fp32 aggregate (reduce_ groups
        # those into one flame_agg_reduce_mx per element format)
        mxk = {k for k in ks if any_mx and mx_route(agg[k].dtype, [entries[ci][0] for ci in cis], k, agg[k].shape) is not None}
        # same: one reduction launch per dtype pair -- the aggregate's own dtype, or bf16 / f16
        # updates under an fp32 aggregate (reduce_ groups those into flame_agg_reduce_mixed)
        same = [k for k in ks if k in mxk or (agg[k].dtype in DTYPE_CODE
                and (all(entries[ci][0][k].dtype == agg[k].dtype for ci in cis)
                     or uplink16_dtype(agg[k].dtype, (entries[ci][0][k].dtype for ci in cis)) is not None))]
        mixed = [k for k in ks if k not in same]
        for k in mixed:     # (a float8 tensor in a plain dict ends here)
            for ci in cis:
                _check_cast(agg[k].dtype, weight_dtype(entries[ci][0], k))
        routed.append((cis, mxk, same, mixed))
    # every refusal of the round has been raised: the aggregate is untouched until here
    for cis, mxk, same, mixed in routed:
        # with clip scales the float keys take the scaled kernel; integer keys are never scaled
        parts = [(same, None)] if scales is None else [
            ([k for k in same if agg[k].is_floating_point()], [scales[ci] for ci in cis]),
            ([k for k in same if not agg[k].is_floating_point()], None)]
        for part, sc in parts:
            if not part:
                continue
            targets = [_Target(agg[k], device) for k in part]
            outs = [t.dev for t in targets]
            clients = [[entries[ci][0][k] for ci in cis] for k in part]
            bsc = [[entries[ci][0].scales[k] for ci in cis] if k in mxk else None for k in part] if mxk else None
            reduce_(outs, outs, clients, [entries[ci][1] for ci in cis], scales=sc, **({} if bsc is None else {"block_scales": bsc}))
            for t in targets:
                t.writeback()
        sub = [entries[ci] for ci in cis]
        if scales is not None and mixed:
            sub = _prescaled(sub, [scales[ci] for ci in cis], mixed, device)
        _accumulate_mixed(agg, mixed, sub, device)


def _prescaled(entries, scales, keys, device):
    """``entries`` restricted to ``keys`` with every float tensor replaced by
    ``round(v * scale)`` in its own dtype (:func:`tmp_of`, the same statement the scaled
    kernel fuses); integer and bool tensors pass through."""
    out = []
    for (w, r), sc in zip(entries, scales):
        d = {}
        for k in keys:
            if k not in w:
                continue
            v = w[k]
            d[k] = tmp_of(v, sc, device, logical_shape(w, k)) if v.is_floating_point() else v
        out.append((d, r))
    return out


class _KeyLike:
    """What :func:`_client_row` reads of an aggregate tensor, for a key that has none here."""

    def __init__(self, numel, dtype):
        self._numel, self.dtype = numel, dtype

    def numel(self):
        return self._numel

    def element_size(self):
        return torch.empty((), dtype=self.dtype).element_size()


def _rows(ws, fkeys, numels, dts, device, keep, per_view=True):
    """``{key: (pointer row, tile stride bytes)}`` of keys every update of ``ws`` carries: from the
    slot numbers when all are slots of ONE UpdateSlab (:func:`slab_rows`, no view touched), else with
    ``per_view`` one :func:`_client_row` per key (``keep``: what must outlive the launch), else None."""
    rows = slab_rows(ws, fkeys, numels, dts, device) if fkeys and getattr(ws[0], "slab", None) is not None else None
    if rows is None and per_view:
        rows = {k: _client_row([w[k] for w in ws], _KeyLike(numels[k], dts[k]), device, keep) for k in fkeys}
    return rows


def _float_items(ws, device, keep, uniform=None, inp=None):
    """The FLOAT keys of the updates ``ws`` as ``(dtype, client indices, Seg)`` items, one per key,
    for the launches that read updates and write no model.  Integer and bool tensors take no part;
    an unsupported float dtype raises (:func:`dtype_code`).  Slots of one UpdateSlab take
    :func:`_rows`' fast path (the first slot's keys stand for all); otherwise every view is looked at:

    * ragged allowed (``uniform`` None, :func:`update_stats`): a ``(key, dtype)`` is measured over
      the updates that carry it, so the client indices may differ between items;
    * uniform required (``uniform`` names the launcher, :func:`update_gram`): every update carries
      every float key in one dtype and shape (a distance between other updates means nothing).

    ``inp(key, dtype, shape)`` (:func:`update_dist`) gives each item's ``Seg.inp``: the address of the
    tensor the kernel reads beside the updates of that key."""
    inp = inp or (lambda k, dt, shape: 0)
    all_cis = tuple(range(len(ws)))
    w0 = ws[0]
    if getattr(w0, "slab", None) is not None:
        fkeys = [k for k in w0.keys() if weight_dtype(w0, k).is_floating_point and weight_dtype(w0, k) in DTYPE_CODE]
        numels = {k: math.prod(logical_shape(w0, k)) for k in fkeys}
        dts = {k: weight_dtype(w0, k) for k in fkeys}
        rows = _rows(ws, fkeys, numels, dts, device, keep, per_view=False)
        if rows is not None:
            return [(dts[k], all_cis, Seg(numels[k], inp=inp(k, dts[k], logical_shape(w0, k)), clients=rows[k][0],
                                          tile_stride=rows[k][1])) for k in fkeys]
    per = collections.OrderedDict()     # first-seen order.  ragged: (key, dtype) -> client indices;
    for ci, w in enumerate(ws):         # uniform: key -> (dtype, shape) of the update that brought it first
        for k in w.keys():
            dt = weight_dtype(w, k)
            if dt.is_floating_point:
                dtype_code(dt)          # an unsupported float dtype raises
                if uniform is None:
                    per.setdefault((k, dt), []).append(ci)
                else:
                    per.setdefault(k, (dt, tuple(logical_shape(w, k))))
    if uniform is None:
        keyed = [(k, dt, logical_shape(ws[cis[0]], k), tuple(cis)) for (k, dt), cis in per.items()]
    else:
        for ci, w in enumerate(ws):
            for k, (dt, shape) in per.items():
                if k not in w:
                    raise ValueError(f"flame_amd.{uniform}: update {ci} lacks the key {k!r} that another update has")
                if weight_dtype(w, k) != dt or tuple(logical_shape(w, k)) != shape:
                    raise ValueError(f"flame_amd.{uniform}: update {ci} holds {k!r} as {weight_dtype(w, k)} "
                                     f"{tuple(logical_shape(w, k))}, another as {dt} {shape}")
        keyed = [(k, dt, shape, all_cis) for k, (dt, shape) in per.items()]
    items = []
    for k, dt, shape, cis in keyed:
        numel = math.prod(shape)
        row, tstride = _client_row([ws[ci][k] for ci in cis], _KeyLike(numel, dt), device, keep)
        items.append((dt, cis, Seg(numel, inp=inp(k, dt, shape), clients=row, tile_stride=tstride)))
    return items


def _measure(kernel, items, device, keep, width):
    """Entry point ``kernel`` (scratch size: ``<kernel>_scratch_bytes``) over :func:`_float_items`'
    items: one launch per (dtype, client set) in first-seen order, every group planned first (no
    rates are read), ONE scratch buffer sized for the largest plan, ONE zeroed int64 output block
    all launches add into, copied back once (that copy waits for the stream).  The block is
    ``[first | second]``, each part by *slot*: one per distinct client set in first-seen order
    (normally one), ``width(n)`` and ``n`` words for ``n`` clients.  Returns the parts (host int64)
    and ``{client set: (first offset, second offset)}``."""
    L = N.lib()
    entry, scratch_bytes = getattr(L, kernel), getattr(L, kernel + "_scratch_bytes")
    one = items[0][1]       # the usual case is ONE client set (the same tuple): no per-item hash of it then
    also = None if all(it[1] is one for it in items) else (lambda it: it[1])
    groups = [(key if also else (key, one), its) for key, its in by_dtype(items, lambda it: it[0], also=also).items()]
    slots, first, second = collections.OrderedDict(), 0, 0      # groups: [((dtype code, client indices), items)]
    for (_, cis), _ in groups:
        if cis not in slots:
            slots[cis] = (first, second)
            first += width(len(cis))
            second += len(cis)
    out = torch.zeros(first + second, dtype=torch.int64, device=device)
    plans = [(code, cis, plan(code, [sg for _, _, sg in its], [0.0] * len(cis)), sum(sg.numel for _, _, sg in its))
             for (code, cis), its in groups]
    sbytes = max(int(scratch_bytes(p.n_chunks, p.n_clients)) for _, _, p, _ in plans)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=device)
    for code, cis, p, elems in plans:
        o1, o2 = slots[cis]
        _launch(kernel, elems * ITEMSIZE[code] * len(cis), device, keep, p.meta,
                lambda b: entry(code, b, p.n_segs, p.n_chunks, b + p.off_clients, p.n_clients,
                                out.data_ptr() + 8 * o1, out.data_ptr() + 8 * (first + o2), scratch.data_ptr(), sbytes,
                                _stream_ptr(device)))
    keep.append(scratch)
    _keepalive(keep, device)
    host = out.cpu().numpy()                    # the one D2H; waits for the launches above
    return host[:first], host[first:], slots


def update_stats(weights_list, device=None):
    """Per update: the sum of squares of its finite float elements and the count of its
    non-finite ones (kernel: flame_update_stats; differential_privacy.py:68-76 takes the square
    root of the former).  Returns ``(sumsq: np.float64[n], nonfinite: np.int64[n])`` in the
    order of ``weights_list``.

    Each update's FLOAT tensors are grouped by their own dtype (:func:`_float_items`, ragged key
    sets allowed) and every dtype is one launch into ``[sumsq as doubles | counts]`` (:func:`_measure`).
    Integer and bool tensors take no part (BatchNorm's ``num_batches_tracked`` is not part of the
    norm).  The call ends with one device-to-host copy of 16 bytes per update, which waits for the
    stream: this is a synchronisation point."""
    ws = list(weights_list)
    n = len(ws)
    sumsq, nonfinite = np.zeros(n, np.float64), np.zeros(n, np.int64)
    if n == 0:
        return sumsq, nonfinite
    refuse_mx(ws, "the update guard's / rfa's measurement (engine.update_stats)")
    device = _hip_device(device, "update_stats", *ws)
    keep = []
    items = _float_items(ws, device, keep)
    if not items:
        return sumsq, nonfinite
    sq, nf, slots = _measure("flame_update_stats", items, device, keep, int)
    sq = sq.view(np.float64)
    for cis, (o, _) in slots.items():
        idx = np.asarray(cis, dtype=np.int64)
        sumsq[idx] += sq[o:o + len(cis)]
        nonfinite[idx] += nf[o:o + len(cis)]
    return sumsq, nonfinite


def update_dist(weights_list, center, device=None):
    """Per update: the squared distance of its finite float elements to ``center`` and the count of
    its non-finite ones (kernel: flame_update_dist, the statistics pass with one fp64 subtract per
    element; the Weiszfeld iterations of ``optimizer/rfa.py`` measure with it).  Returns
    ``(dist2: np.float64[n], nonfinite: np.int64[n])`` in the order of ``weights_list``.

    :func:`update_stats`' front end and ragged-key policy; ``center`` is a dict that must hold every
    float key the updates carry, in that key's dtype and shape (ValueError naming the key
    otherwise).  A centre tensor on the host or with strides is staged to the device first; a
    misaligned one is read element by element, as misaligned updates are.  A non-finite update
    element adds nothing and is counted; a non-finite centre element makes the distance of every
    update that is finite there ``+inf`` or NaN and is not counted.  With an all-zero centre the
    result is :func:`update_stats`' bit for bit.  The call ends with one device-to-host copy of 16
    bytes per update, which waits for the stream: this is a synchronisation point."""
    ws = list(weights_list)
    n = len(ws)
    dist2, nonfinite = np.zeros(n, np.float64), np.zeros(n, np.int64)
    if n == 0:
        return dist2, nonfinite
    refuse_mx(ws, "rfa's measurement (engine.update_dist)")
    device = _hip_device(device, "update_dist", *ws)
    keep = []

    def centre(k, dt, shape):
        if k not in center:
            raise ValueError(f"flame_amd.update_dist: center lacks the float key {k!r} that an update carries")
        z = center[k]
        if z.dtype != dt or tuple(z.shape) != tuple(shape):
            raise ValueError(f"flame_amd.update_dist: center holds {k!r} as {z.dtype} {tuple(z.shape)}, "
                             f"an update as {dt} {tuple(shape)}")
        z = _staged(z, device)
        keep.append(z)
        return z.data_ptr()

    items = _float_items(ws, device, keep, inp=centre)
    if not items:
        return dist2, nonfinite
    d2, nf, slots = _measure("flame_update_dist", items, device, keep, int)
    d2 = d2.view(np.float64)
    for cis, (o, _) in slots.items():
        idx = np.asarray(cis, dtype=np.int64)
        dist2[idx] += d2[o:o + len(cis)]
        nonfinite[idx] += nf[o:o + len(cis)]
    return dist2, nonfinite


def gram_max_clients() -> int:
    """The most updates one Gram launch takes (flame_update_gram_max_clients)."""
    return int(N.lib().flame_update_gram_max_clients())


def update_gram(weights_list, device=None):
    """The pairwise Gram matrix of the updates over their sanitised float elements, and each
    update's non-finite count (kernel: flame_update_gram, fp64 matrix cores; Krum / Multi-Krum's
    distances come from it, ``optimizer/krum.py``).  Returns ``(gram: np.float64[n, n],
    nonfinite: np.int64[n])`` in the order of ``weights_list``; ``gram[i][i]`` is
    :func:`update_stats`' ``sumsq[i]`` up to summation order.

    :func:`update_stats`' front end under :func:`_float_items`' other policy: every update must carry
    every float key in one dtype and shape (ValueError naming the key), so there is one slot,
    ``[n * n gram as doubles | n counts]``.  The call ends with one device-to-host copy of
    ``8 n (n + 1)`` bytes, which waits for the stream: this is a synchronisation point."""
    ws = list(weights_list)
    n = len(ws)
    if n == 0:
        return np.zeros((0, 0), np.float64), np.zeros(0, np.int64)
    if n > gram_max_clients():
        raise NotImplementedError(f"flame_amd.update_gram: {n} updates exceed the kernel's capacity of {gram_max_clients()}")
    refuse_mx(ws, "krum's measurement (engine.update_gram)")
    device = _hip_device(device, "update_gram", *ws)
    keep = []
    items = _float_items(ws, device, keep, uniform="update_gram")
    if not items:
        return np.zeros((n, n), np.float64), np.zeros(n, np.int64)
    gram, nf, _ = _measure("flame_update_gram", items, device, keep, lambda n_cl: n_cl * n_cl)
    return gram.view(np.float64).reshape(n, n).copy(), nf.copy()


def trimmed_max_k() -> int:
    """The largest trim count the kernels carry (flame_agg_trimmed_max_k)."""
    return int(N.lib().flame_agg_trimmed_max_k())


def trimmed_mean(agg: dict, weights_list, k: int, *, init_first: bool = False, device=None) -> None:
    """agg[key] += the coordinate-wise ``k``-trimmed mean of the updates, in place (kernel:
    flame_agg_trimmed; Yin et al., ICML 2018 -- flame has no counterpart).  Per element the ``k``
    smallest and ``k`` largest of the ``n`` values are dropped (NaN sorts last, as ``torch.sort``
    places it), the rest are summed in fp64 in their streaming order and divided by ``n - 2k``;
    ``k = (n - 1) // 2`` is the median, ``k = 0`` the unweighted mean.  With ``init_first`` the
    mean itself is written and the aggregate is not read.  DESIGN.md §2 states the contract.

    Float keys (f32 / bf16 / f16 / f64) are grouped by dtype, one launch each; every update must
    carry exactly the aggregate's float keys in the aggregate's dtypes (ValueError otherwise).
    Integer / bool / narrow keys (``num_batches_tracked``, masks) are not trimmed: they take the
    existing statement with equal weights, ``accumulate`` with rate ``1 / n`` -- no robustness is
    claimed for counters.  Counts play no part: a weighted trimmed mean would let a liar choose
    its own weight.  The updates are only read."""
    def capacity(n, k):
        if k > trimmed_max_k():
            raise NotImplementedError(f"trimmed_mean: k = {k} exceeds the kernels' chain capacity {trimmed_max_k()}")
    _trimmed("trimmed_mean", "flame_agg_trimmed", capacity, agg, weights_list, k, init_first, device)


def select_max_clients() -> int:
    """The most updates a selected round takes (flame_agg_select_max_clients)."""
    return int(N.lib().flame_agg_select_max_clients())


def selected_mean(agg: dict, weights_list, k: int, *, init_first: bool = False, device=None) -> None:
    """``trimmed_mean`` for any ``k`` with ``n > 2k`` (kernel: flame_agg_select): the two order
    statistics that bound the kept values are found per element by a radix search over the keys,
    the values strictly between them are summed in fp64 in client order and the ties at both ends
    enter as count x value.  The kept multiset is ``trimmed_mean``'s; the order of
    the fp64 adds is not, so the two can differ in the last bit where the sum is inexact.  ``n`` is
    at most ``select_max_clients()`` (NotImplementedError beyond).  Grouping, checks and the
    integer / bool / narrow keys are ``trimmed_mean``'s."""
    def capacity(n, k):
        if n > select_max_clients():
            raise NotImplementedError(f"selected_mean: {n} updates exceed the selection kernel's capacity of "
                                      f"{select_max_clients()} (select_max_clients)")
    _trimmed("selected_mean", "flame_agg_select", capacity, agg, weights_list, k, init_first, device)


def _trimmed(who, symbol, capacity, agg, weights_list, k, init_first, device) -> None:
    """The one body of ``trimmed_mean`` and ``selected_mean``: checks, grouping, plan / stage / launch."""
    ws = list(weights_list)
    n = len(ws)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"{who}: k must be an int, not {type(k).__name__}")
    k = int(k)
    refuse_mx(representatives(ws), f"trim (engine.{who})")
    if k < 0 or n <= 2 * k:
        raise ValueError(f"{who}: need 0 <= k and n > 2k, got k = {k} with {n} update(s)")
    capacity(n, k)
    fkeys = [key for key, t in agg.items() if t.is_floating_point()]
    others = [key for key in agg if key not in fkeys]
    want = {key: agg[key].dtype for key in fkeys}
    for w in representatives(ws):
        have = {key: weight_dtype(w, key) for key in w.keys()}
        if {key for key, dt in have.items() if dt.is_floating_point} != set(fkeys) or \
                any(have[key] != dt for key, dt in want.items()):
            raise ValueError(f"{who}: every update must carry the aggregate's float keys in the aggregate's dtypes")
    if init_first and others:
        raise ValueError(f"{who}: init_first covers float keys only; {others!r} need a base")
    device = _hip_device(device, who, *ws, prefer=agg)
    if fkeys:
        for key in fkeys:
            dtype_code(want[key])               # an unsupported float dtype raises
        targets = {key: _Target(agg[key], device) for key in fkeys}
        numels = {key: agg[key].numel() for key in fkeys}
        keep = []
        rows = _rows(ws, fkeys, numels, want, device, keep)
        L = N.lib()
        for code, ks in by_dtype(fkeys, lambda key: want[key]).items():
            segs = []
            for key in ks:
                o = targets[key].dev
                row, tstride = rows[key]
                segs.append(Seg(o.numel(), out=o.data_ptr(), inp=0 if init_first else o.data_ptr(), clients=row,
                                tile_stride=tstride))
            p = plan(code, segs, [0.0] * n)     # the kernel reads no rates: today's block, as update_stats builds it
            flags = N.FLAME_AGG_INIT_FIRST if init_first else 0
            if p.n_chunks >= XCD_MAP_MIN_CHUNKS and all(s.tile_stride == 0 for s in segs):
                flags |= N.FLAME_AGG_XCD_MAP
            nbytes = sum(s.numel for s in segs) * ITEMSIZE[code] * (n + (1 if init_first else 2))
            _launch(symbol, nbytes, device, keep, p.meta,
                    lambda b: getattr(L, symbol)(code, flags, b, p.n_segs, p.n_chunks, b + p.off_clients, p.n_clients,
                                                  k, _stream_ptr(device)))
        _keepalive(keep, device)
        for t in targets.values():
            t.writeback()
    if others:
        accumulate({key: agg[key] for key in others},
                   [({key: w[key] for key in others if key in w}, 1.0 / n) for w in ws], device=device)


def weight_dtype(weights, k) -> torch.dtype:
    """dtype of ``weights[k]`` without making a view (slab slots know it from the slab)."""
    slab = getattr(weights, "slab", None)
    if slab is not None:
        rng = getattr(weights, "ranges", None)
        return slab.meta[rng[k][0] if rng is not None else k][0]
    return weights[k].dtype


def representatives(ws):
    """One weights dict per distinct layout among ``ws``: slots of one slab (sharing one
    ``ranges`` table) all carry the same keys and dtypes, so one of them stands for all;
    any other dict stands for itself.  Lets per-key dtype checks skip thousands of slots."""
    seen, out = set(), []
    for w in ws:
        slab = getattr(w, "slab", None)
        if slab is not None:
            tag = (id(slab), id(getattr(w, "ranges", None)), len(w))
            if tag in seen:
                continue
            seen.add(tag)
        out.append(w)
    return out


def slab_rows(ws, keys, numels, dtypes, device):
    """Pointer rows of ``keys`` for client weights ``ws`` that all live in ONE UpdateSlab:
    every ``w`` a whole :class:`~flame_amd.slab.SlotWeights` of the slab, or every ``w`` a
    :class:`~flame_amd.slab.SlabRef` sharing one ``ranges`` table.  Addresses come from the
    slot numbers (numpy), no per-client view is touched.  Returns ``{k: (uint64 pointers in
    ``ws`` order, tile stride bytes)}``, or None when the case does not apply (the caller
    then takes the per-view path)."""
    if not ws:
        return None
    first = ws[0]
    slab = getattr(first, "slab", None)
    if slab is None or slab.device != device:
        return None
    ranges = getattr(first, "ranges", None)
    nk = len(slab.keys)
    for w in ws:
        if getattr(w, "slab", None) is not slab or getattr(w, "ranges", None) is not ranges:
            return None
        if ranges is None and len(w) != nk:
            return None
    slots = np.fromiter((w.slot for w in ws), dtype=np.uint64, count=len(ws))
    return slot_rows(slab, ranges, slots, keys, numels, dtypes, device)


def slot_rows(slab, ranges, slots, keys, numels, dtypes, device):
    """:func:`slab_rows` from slot numbers already known (``slots``: uint64, client order) of
    ``slab`` (whole slots with ``ranges`` None, or one shared ``ranges`` table)."""
    if slab.device != device:
        return None
    rows = {}
    for k in keys:
        if ranges is not None:
            if k not in ranges:
                return None
            key, lo, hi = ranges[k]
        else:
            if k not in slab.meta:
                return None
            key, lo, hi = k, 0, slab.meta[k][2]
        dt, _, base, slot_bytes, tile_bytes = slab.key_layout(key)
        T = slab.storage[dt].shape[2]
        if dt != dtypes[k] or hi - lo != numels[k] or lo % T:
            return None
        rows[k] = (np.uint64(base + (lo // T) * tile_bytes) + slots * np.uint64(slot_bytes), tile_bytes)
    return rows


def _accumulate_slab(agg: dict, entries, device, key_groups=None, after_group=None, scales=None) -> bool:
    """Fast path: every entry lives in ONE UpdateSlab (whole slots, or :class:`SlabRef`
    ranges sharing one table) and carries exactly agg's keys in agg's dtypes.  Pointer rows
    are computed from slot numbers (numpy), without touching the per-client views; returns
    False (nothing done) when the case does not apply."""
    w0 = entries[0][0]
    if getattr(w0, "slab", None) is None or len(w0) != len(agg):
        return False
    # the slab's dtype of a key may be bf16 / f16 under an fp32 aggregate (flame_agg_reduce_mixed)
    dts = {}
    for k in agg:
        dts[k] = agg[k].dtype
        if dts[k] == torch.float32:
            try:
                dts[k] = uplink16_dtype(dts[k], (weight_dtype(w0, k),)) or dts[k]
            except KeyError:
                return False
    rows = slab_rows([w for w, _ in entries], list(agg.keys()), {k: agg[k].numel() for k in agg}, dts, device)
    if rows is None:
        return False
    rates = [r for _, r in entries]
    targets = {k: _Target(agg[k], device) for k in agg.keys()}
    keep = []
    for gi, g in enumerate(key_groups if key_groups is not None else [list(agg.keys())]):
        for (code, ccode), ks in by_dtype(g, lambda k: agg[k].dtype, also=lambda k: dtype_code(dts[k])).items():
            segs = []
            for k in ks:
                ptrs, tile_bytes = rows[k]
                o = targets[k].dev
                segs.append(Seg(o.numel(), out=o.data_ptr(), inp=o.data_ptr(), clients=ptrs, tile_stride=tile_bytes))
            _launch_reduce(code, segs, rates, device, keep, scales=scales if code in FLOAT_CODES else None, ccode=ccode)
        if after_group is not None:
            after_group(gi)
    _keepalive(keep, device)
    for t in targets.values():
        t.writeback()
    return True


def _accumulate_mixed(agg: dict, keys, entries, device) -> None:
    """:func:`_accumulate_promoted` for many keys at once: each key's whole arrival loop
    (``tmp = (v * rate).to(v.dtype); agg[k] += tmp`` per entry, fedavg.py:93-104 /
    fedbuff.py:147-157) is ONE flame_elementwise program written in place into agg[k], and the
    keys whose dtypes / 0-dim-ness agree share one program and one launch (e.g. a ResNet's 53
    BatchNorm ``num_batches_tracked``: int64 updates into the fp32 aggregate FedOPT's promotion
    left).  Aggregates that are not contiguous device tensors, and entries holding tiled slab
    slots, take the per-key path."""
    from . import elementwise as ew
    rates = tuple(float(r) for _, r in entries)
    groups = collections.OrderedDict()
    for k in keys:
        acc = agg[k]
        vs = [w[k] for w, _ in entries]
        for v in vs:
            _check_cast(acc.dtype, v.dtype)
        if (not (acc.is_cuda and acc.device == device and acc.is_contiguous())
                or any(tuple(v.shape) != tuple(acc.shape) for v in vs) or len(vs) > ew.MAX_BUFS - 2):
            _accumulate_promoted(agg, k, entries, device)
            continue
        sig = (acc.dtype, acc.dim() == 0, tuple((v.dtype, v.dim() == 0) for v in vs), rates)
        groups.setdefault(sig, []).append(k)
    for sig, ks in groups.items():
        def stmt(acc, *vs):
            for v, r in zip(vs, rates):
                tmp = v * r
                acc = (acc + tmp.to(v.dtype)).to(acc.dtype)       # agg[k] += tmp, in place
            return acc
        k0 = ks[0]
        specs = [(agg[k0].dtype, tuple(agg[k0].shape))] + [(w[k0].dtype, tuple(w[k0].shape)) for w, _ in entries]
        try:
            prog = ew.cached(("accumulate",) + sig, stmt, specs)
        except NotImplementedError:      # a statement longer than one program: per key, as before
            for k in ks:
                _accumulate_promoted(agg, k, entries, device)
            continue
        prog.run_many([[agg[k]] + [w[k] for w, _ in entries] for k in ks], device, into=[[agg[k]] for k in ks])


def _accumulate_promoted(agg: dict, k, entries, device) -> None:
    """agg[k] += tmp_i where tmp_i = (v_i * rate_i).to(v_i.dtype) has another dtype than
    agg[k], or either is a dtype the kernels do not carry (:data:`NARROW`).

    Each tmp_i is formed in its own dtype (fedavg.py:93-102, :func:`tmp_of`), then added
    with torch's in-place semantics (:104): the sum in promote_types(acc, tmp), rounded back
    to acc's dtype -- :func:`_add_promoted` (integer aggregates: exact integer adds).  Runs
    of tmps whose promotion is acc's own float dtype (e.g. an fp32 aggregate receiving int64
    ``num_batches_tracked``) are summed in one launch: ``fl(acc + T(tmp))`` ==
    ``fl(acc + fl(T(tmp) * 1.0))``.
    """
    acc = agg[k]
    direct = acc.dtype in DTYPE_CODE
    terms = []                   # (tensor, rate, summable by the kernel into acc)
    for w, r in entries:
        v = w[k]
        _check_cast(acc.dtype, v.dtype)
        tmp = tmp_of(v, r, device, acc.shape)
        p = torch.promote_types(acc.dtype, tmp.dtype)
        if direct and p == acc.dtype and p.is_floating_point:    # integers: exact adds below
            terms.append((tmp if tmp.dtype == acc.dtype else tmp.to(acc.dtype), 1.0, True))
        else:
            terms.append((tmp, None, False))
    target = _Target(acc, device)
    run, run_r = [], []

    def flush_run():
        if run:
            reduce_([target.dev], [target.dev], [list(run)], list(run_r))
            run.clear()
            run_r.clear()
    for t, r, summable in terms:
        if summable:
            run.append(t)
            run_r.append(r)
        else:
            flush_run()
            _add_promoted(target.dev, t)
    flush_run()
    target.writeback()


def tmp_of(v: torch.Tensor, rate: float, device, shape=None) -> torch.Tensor:
    """``(v * rate).to(v.dtype)`` (fedavg.py:93-102) as a new device tensor.  Kernel dtypes:
    one init-first launch.  bool / uint8 / int8 / int16: ``v * rate`` is in torch's default
    dtype (fp32: the integral tensor and the rate both cast to it), formed by that dtype's kernel, then
    cast to v's dtype on the device (bool: != 0; integers: truncation -- in range, as
    ``|v * rate| <= |v|`` for the callers' rates <= 1).  ``shape``: the key's model shape
    (``v`` may be a tiled slab view)."""
    shape = v.shape if shape is None else shape
    if v.dtype in DTYPE_CODE:
        tmp = torch.empty(shape, dtype=v.dtype, device=device)
        reduce_([tmp], None, [[v]], [rate], init_first=True)
        return tmp
    if v.dtype not in NARROW:
        dtype_code(v.dtype)          # raises: unsupported (complex, fp8, ...)
    # torch computes an integral tensor times a Python float in the DEFAULT dtype (fp32 unless
    # torch.set_default_dtype changed it; fp64 then uses the rate unrounded)
    ft = torch.get_default_dtype()
    vf = v.to(device).to(ft)
    tf = torch.empty(shape, dtype=ft, device=device)
    reduce_([tf], None, [[vf]], [rate], init_first=True)
    return tf.to(v.dtype)


def _check_cast(acc_dt, v_dt) -> None:
    if v_dt in MX_CODE or acc_dt in MX_CODE:
        raise TypeError(f"flame_amd: a {v_dt if v_dt in MX_CODE else acc_dt} tensor outside an MX update: a float8 / float4 tensor "
                        f"means nothing without its block scales.  {MX_SUPPORTED}")
    p = torch.promote_types(acc_dt, v_dt)
    if not torch.can_cast(p, acc_dt):
        raise RuntimeError(f"result type {str(p).replace('torch.', '').capitalize()} can't be cast to the "
                           f"desired output type {str(acc_dt).replace('torch.', '').capitalize()}")


def _add_promoted(acc: torch.Tensor, tmp: torch.Tensor) -> None:
    """``acc += tmp`` in place with torch's semantics when the dtypes differ: computed in
    promote_types(acc, tmp) and rounded back to acc's dtype (bf16 += f32, f16 += bf16,
    f32 += f64, ...; integer promotions such as int32 += int64 wrap like torch's) -- one
    flame_elementwise launch (casts, the add, the cast back)."""
    from . import elementwise as ew
    _check_cast(acc.dtype, tmp.dtype)
    ew.iadd(acc, ew.Lazy.of(tmp))


def logical_shape(weights, k):
    """Shape of ``weights[k]`` as the model sees it (slab slots hand out tiled views)."""
    shapes = getattr(weights, "shapes", None)
    if shapes is not None and k in shapes:
        return shapes[k]
    return weights[k].shape


def logical_tensor(weights, k) -> torch.Tensor:
    """``weights[k]`` in its logical shape (a tiled slab view is untiled into a copy)."""
    v = weights[k]
    shape = tuple(logical_shape(weights, k))
    if tuple(v.shape) == shape:
        return v
    return v.reshape(-1)[:math.prod(shape)].reshape(shape)


def first_tmp(weights: dict, rate: float, *, device=None) -> dict:
    """{k: round(v[k] * rate)} as new device tensors (fedbuff.py:139-140,154-155)."""
    device = device or pick_device(weights)
    out = collections.OrderedDict()
    ks = list(weights.keys())
    kern = [k for k in ks if weight_dtype(weights, k) in DTYPE_CODE]
    for k in ks:
        if k in kern:
            out[k] = torch.empty(logical_shape(weights, k), dtype=weight_dtype(weights, k), device=device)
        else:
            out[k] = tmp_of(weights[k], rate, device, logical_shape(weights, k))
    if kern:
        reduce_([out[k] for k in kern], None, [[weights[k]] for k in kern], [rate], init_first=True)
    return out
