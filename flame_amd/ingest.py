"""Ingest path: channel payload -> tensors -> aggregation.

flame's channel decodes every received message with ``cloudpickle.loads``
(``lib/python/flame/channel.py:321-325``).  For a model update that pickle is a
dict whose tensors are ``torch._utils._rebuild_tensor_v2(
torch.storage._load_from_bytes(BINBYTES <legacy torch.save stream>), ...)``
(SURVEY.md §3.4); ``loads`` copies every storage at least twice and parses it
through ``torch.load`` -- measured 0.87 GB/s for a 100 MB update, the dominant
host cost of the reference aggregator.

:func:`decode` is a *restricted, zero-copy* decoder for those payloads:

* a small pickle VM (protocols 2-5) that executes NOTHING but an allowlist
  (tensor rebuild, storage load, OrderedDict, flame's ``MessageType`` enum and
  plain containers / scalars) -- any other global raises ``UnpicklingError``,
  which is strictly safer than the reference's unrestricted ``loads``;
* the legacy storage stream is parsed in place and every tensor becomes a
  ``torch.frombuffer`` view into the payload buffer: no byte of tensor data is
  copied on the host.

If the payload lives in pinned / ``hipHostRegister``-ed memory the views are
device-addressable and the reduction kernel streams them straight over PCIe
(``engine.ZERO_COPY_PINNED``); otherwise ``engine`` stages them H2D.
:class:`DeviceUpdateCache` is a ``diskcache.Cache`` stand-in for the aggregator
roles (``syncfl/top_aggregator.py:93-95``) that keeps updates resident in HBM
(or in pinned host memory) instead of pickling them to disk.
"""
from __future__ import annotations

import collections
import enum
import functools
import os
import pickle
import re
import struct
import warnings
from typing import Any, Dict

import torch


# ------------------------------------------------------------------ legacy storage stream
_STORAGE_DTYPES = {
    "FloatStorage": torch.float32, "DoubleStorage": torch.float64, "HalfStorage": torch.float16,
    "BFloat16Storage": torch.bfloat16, "LongStorage": torch.int64, "IntStorage": torch.int32,
    "ShortStorage": torch.int16, "CharStorage": torch.int8, "ByteStorage": torch.uint8,
    "BoolStorage": torch.bool,
}
LEGACY_MAGIC = 0x1950A86A20F9469CFC6C


class _StorageRef:
    """A storage found in the payload: dtype + element count + where its bytes are."""

    __slots__ = ("buf", "offset", "numel", "dtype")

    def __init__(self, buf, offset, numel, dtype):
        self.buf, self.offset, self.numel, self.dtype = buf, offset, numel, dtype

    def tensor(self) -> torch.Tensor:
        if self.numel == 0:
            return torch.empty(0, dtype=self.dtype)
        return torch.frombuffer(self.buf, dtype=self.dtype, count=self.numel, offset=self.offset)


class _PersistentStorage:
    def __init__(self, dtype, key, numel):
        self.dtype, self.key, self.numel = dtype, key, numel


# ------------------------------------------------------------------ restricted pickle VM
def _rebuild_tensor_v2(storage, storage_offset, size, stride, requires_grad=False, backward_hooks=None,
                       metadata=None):
    if not isinstance(storage, _StorageRef):
        raise pickle.UnpicklingError("tensor rebuild without a storage")
    t = storage.tensor()
    if not (storage_offset == 0 and len(size) == 1 and size[0] == storage.numel and tuple(stride) == (1,)):
        t = t.as_strided(tuple(size), tuple(stride), storage_offset)     # (a whole 1-D storage is `t` itself)
    # the payload buffer the view reads: UpdateSlab.write copies one update's tensors that
    # share a payload with ONE host->device transfer (flame_amd/slab.py)
    t._flame_payload = storage.buf
    return t


class PayloadDecoder:
    """Restricted pickle VM over a buffer; see module docstring."""

    def __init__(self, buf, extra_globals: Dict[tuple, Any] = None):
        self.mv = memoryview(buf).cast("B")
        self.buf = buf
        self.globals = dict(_default_globals())
        if extra_globals:
            self.globals.update(extra_globals)

    # -- helpers
    def _unpack(self, fmt, p):
        n = struct.calcsize(fmt)
        return struct.unpack_from(fmt, self.mv, p)[0], p + n

    def load(self, pos=0, persistent_load=None):
        """Run one pickle starting at ``pos``; return (object, end position).  The opcode loop
        is the C one (``csrc/pickle_vm.c``, same opcodes, same allowlist calls) unless
        ``FLAME_AMD_PICKLE_VM=py`` selects :meth:`load_py`."""
        if _VM is None:
            return self.load_py(pos, persistent_load)
        return _VM.load(self.mv, pos, self._find, self._call, _Span, persistent_load, _load_from_bytes_marker)

    def load_py(self, pos=0, persistent_load=None):
        """The opcode loop in Python (the C loop's specification; differential-tested)."""
        mv = self.mv
        stack, memo, marks = [], {}, []
        push, pop, call = stack.append, stack.pop, self._call     # (hot loop: locals, not attributes)
        p = pos
        while True:
            op = mv[p]
            p += 1
            # opcodes in order of frequency in update payloads (MEMOIZE, BININT1, REDUCE, ... first)
            if op == 0x94:    # MEMOIZE
                memo[len(memo)] = stack[-1]
            elif op == 0x4B:    # BININT1
                push(mv[p])
                p += 1
            elif op == 0x52:    # REDUCE
                args = pop()
                stack[-1] = call(stack[-1], args)
            elif op == 0x68:    # BINGET
                push(memo[mv[p]])
                p += 1
            elif op == 0x8C:    # SHORT_BINUNICODE
                n = mv[p]
                push(str(mv[p + 1:p + 1 + n], "utf-8"))
                p += 1 + n
            elif op == 0x85:    # TUPLE1
                stack[-1] = (stack[-1],)
            elif op == 0x28:    # MARK
                marks.append(len(stack))
            elif op == 0x74:    # TUPLE
                k = marks.pop()
                if k > len(stack):
                    raise IndexError("stack underflow below MARK")
                stack[k:] = [tuple(stack[k:])]
            elif op in (0x43, 0x42, 0x8E):  # SHORT_BINBYTES, BINBYTES, BINBYTES8: keep a SPAN, no copy
                if op == 0x43:
                    n = mv[p]
                    p += 1
                elif op == 0x42:
                    n = int.from_bytes(mv[p:p + 4], "little")
                    p += 4
                else:
                    n = int.from_bytes(mv[p:p + 8], "little")
                    p += 8
                # the argument of torch.storage._load_from_bytes (on top of the stack): a span
                # of the payload, no copy; any other bytes value is a bytes object
                push(_Span(p, n) if stack and stack[-1] is _load_from_bytes_marker else bytes(mv[p:p + n]))
                p += n
            elif op == 0x96:    # BYTEARRAY8 (protocol 5)
                n = int.from_bytes(mv[p:p + 8], "little")
                p += 8
                if p + n > len(mv):
                    raise IndexError("truncated")
                push(bytearray(mv[p:p + n]))
                p += n
            elif op == 0x29:    # EMPTY_TUPLE
                push(())
            elif op == 0x89:    # NEWFALSE
                push(False)
            elif op == 0x80:      # PROTO
                p += 1
            elif op == 0x95:    # FRAME
                p += 8
            elif op == 0x2E:    # STOP
                return stack.pop(), p
            elif op == 0x7D:    # EMPTY_DICT
                stack.append({})
            elif op == 0x5D:    # EMPTY_LIST
                stack.append([])
            elif op == 0x8F:    # EMPTY_SET
                stack.append(set())
            elif op == 0x71:    # BINPUT
                memo[mv[p]] = stack[-1]
                p += 1
            elif op == 0x72:    # LONG_BINPUT
                i, p = self._unpack("<I", p)
                memo[i] = stack[-1]
            elif op == 0x6A:    # LONG_BINGET
                i, p = self._unpack("<I", p)
                stack.append(memo[i])
            elif op == 0x58:    # BINUNICODE
                n, p = self._unpack("<I", p)
                stack.append(bytes(mv[p:p + n]).decode("utf-8"))
                p += n
            elif op == 0x8D:    # BINUNICODE8
                n, p = self._unpack("<Q", p)
                stack.append(bytes(mv[p:p + n]).decode("utf-8"))
                p += n
            elif op == 0x4D:    # BININT2
                v, p = self._unpack("<H", p)
                stack.append(v)
            elif op == 0x4A:    # BININT
                v, p = self._unpack("<i", p)
                stack.append(v)
            elif op == 0x8A:    # LONG1
                n = mv[p]
                stack.append(int.from_bytes(bytes(mv[p + 1:p + 1 + n]), "little", signed=True))
                p += 1 + n
            elif op == 0x47:    # BINFLOAT
                v, p = self._unpack(">d", p)
                stack.append(v)
            elif op == 0x4E:    # NONE
                stack.append(None)
            elif op == 0x88:    # NEWTRUE
                stack.append(True)
            elif op == 0x86 or op == 0x87:    # TUPLE2, TUPLE3
                k = len(stack) - (op - 0x84)
                if k < 0:
                    raise IndexError("stack underflow")
                stack[k:] = [tuple(stack[k:])]
            elif op == 0x91:    # FROZENSET
                k = marks.pop()
                if k > len(stack):
                    raise IndexError("stack underflow below MARK")
                stack[k:] = [frozenset(stack[k:])]
            elif op == 0x6C:    # LIST
                k = marks.pop()
                if k > len(stack):
                    raise IndexError("stack underflow below MARK")
                stack[k:] = [list(stack[k:])]
            elif op == 0x65:    # APPENDS
                k = marks.pop()
                if k > len(stack):
                    raise IndexError("stack underflow below MARK")
                items = stack[k:]
                del stack[k:]
                stack[-1].extend(items)
            elif op == 0x61:    # APPEND
                v = stack.pop()
                stack[-1].append(v)
            elif op == 0x75:    # SETITEMS
                k = marks.pop()
                if k > len(stack):
                    raise IndexError("stack underflow below MARK")
                items = stack[k:]
                del stack[k:]
                d = stack[-1]
                for i in range(0, len(items), 2):
                    d[items[i]] = items[i + 1]
            elif op == 0x73:    # SETITEM
                v = stack.pop()
                key = stack.pop()
                stack[-1][key] = v
            elif op == 0x90:    # ADDITEMS
                k = marks.pop()
                if k > len(stack):
                    raise IndexError("stack underflow below MARK")
                items = stack[k:]
                del stack[k:]
                stack[-1].update(items)
            elif op == 0x93:    # STACK_GLOBAL
                name = stack.pop()
                module = stack.pop()
                stack.append(self._find(module, name))
            elif op == 0x63:    # GLOBAL (text "module\nname\n")
                e1 = bytes(mv[p:p + 256]).index(b"\n")
                module = bytes(mv[p:p + e1]).decode()
                e2 = bytes(mv[p + e1 + 1:p + e1 + 257]).index(b"\n")
                name = bytes(mv[p + e1 + 1:p + e1 + 1 + e2]).decode()
                p += e1 + e2 + 2
                stack.append(self._find(module, name))
            elif op == 0x81:    # NEWOBJ
                args = stack.pop()
                cls = stack.pop()
                stack.append(self._call(cls, args))
            elif op == 0x62:    # BUILD (only trivial state on allowlisted objects)
                state = stack.pop()
                if state:
                    raise pickle.UnpicklingError("BUILD with state is not allowed in update payloads")
            elif op == 0x51:    # BINPERSID
                pid = stack.pop()
                if persistent_load is None:
                    raise pickle.UnpicklingError("persistent id outside a storage stream")
                stack.append(persistent_load(pid))
            else:
                raise pickle.UnpicklingError(f"opcode 0x{op:02x} not allowed in update payloads")

    def _find(self, module, name):
        try:
            return self.globals[(module, name)]
        except KeyError:
            raise pickle.UnpicklingError(f"global {module}.{name} is not allowed in update payloads") from None

    def _call(self, fn, args):
        if fn is _load_from_bytes_marker:
            (span,) = args
            if isinstance(span, (bytes, bytearray)):  # protocol <= 2 carries bytes as _codecs.encode(str)
                sub = PayloadDecoder(span)
                return sub._storage_from_span(_Span(0, len(span)))
            return self._storage_from_span(span)
        if not getattr(fn, "_flame_amd_allowed", False) and fn not in _CALLABLE_ALLOW:
            raise pickle.UnpicklingError(f"call of {fn!r} not allowed")
        return fn(*args)

    def _storage_from_span(self, span):
        """Parse the legacy torch.save stream inside the payload (no copy)."""
        if not isinstance(span, _Span):
            raise pickle.UnpicklingError("storage bytes expected")
        q = span.start
        if _VM is not None and _STORAGE_HEADERS:
            # the common case in C: a validated header, then torch's record layout (the same
            # checks as below; None = anything else, parsed the long way)
            hit = _VM.storage_head(self.mv, q, span.start + span.n, _STORAGE_HEADERS)
            if hit is not None:
                dtype = _STORAGE_DTYPES.get(hit[0])
                if dtype is not None:
                    numel, q = hit[1], hit[2]
                    if q + numel * dtype.itemsize > span.start + span.n:
                        raise pickle.UnpicklingError("storage runs past its bytes")
                    return _StorageRef(self.buf, q, numel, dtype)
        # magic, protocol and sys-info pickles: the same bytes before every storage of a
        # payload, so a header already parsed and checked is skipped by a byte compare
        for h in _STORAGE_HEADERS:
            if self.mv[q:q + len(h)] == h:
                q += len(h)
                break
        else:
            magic, q = self.load(q)
            if magic != LEGACY_MAGIC:
                raise pickle.UnpicklingError("not a legacy torch storage stream")
            _proto, q = self.load(q)
            _sysinfo, q = self.load(q)
            if len(_STORAGE_HEADERS) < 8:
                _STORAGE_HEADERS.append(bytes(self.mv[span.start:q]))
        # torch's own record layout (legacy _save, protocol 2): parsed field by field, every byte
        # checked; the storage key inside it is the storage's address, new in every message
        rec = _parse_storage_record(self.mv, q)
        if rec is not None:
            dtype, numel, q = rec
            nbytes = numel * dtype.itemsize
            if q + nbytes > span.start + span.n:
                raise pickle.UnpicklingError("storage runs past its bytes")
            return _StorageRef(self.buf, q, numel, dtype)
        # any other encoding of the record: parse results kept by the record's exact bytes (the
        # VM is a pure function of them), grouped by record length
        for n_rec, seen in _STORAGE_RECORDS.items():
            hit = seen.get(bytes(self.mv[q:q + n_rec]))
            if hit is not None:
                dtype, numel, nbytes = hit
                q += n_rec
                if q + nbytes > span.start + span.n:
                    raise pickle.UnpicklingError("storage runs past its bytes")
                return _StorageRef(self.buf, q, numel, dtype)
        rec0 = q
        found = []

        def pload(pid):
            # ('storage', storage_type, root_key, location, numel[, view_metadata])
            if not isinstance(pid, tuple) or pid[0] != "storage":
                raise pickle.UnpicklingError("unexpected persistent id")
            st = pid[1]
            ps = _PersistentStorage(st, pid[2], int(pid[4]))
            found.append(ps)
            return ps
        obj, q = self.load(q, persistent_load=pload)
        keys, q = self.load(q)
        if not isinstance(obj, _PersistentStorage) or len(keys) != 1:
            raise pickle.UnpicklingError("expected exactly one storage")
        numel, q = self._unpack("<q", q)
        if numel != obj.numel:
            raise pickle.UnpicklingError("storage size mismatch")
        nbytes = numel * torch.empty(0, dtype=obj.dtype).element_size()
        if q + nbytes > span.start + span.n:
            raise pickle.UnpicklingError("storage runs past its bytes")
        _remember_record(bytes(self.mv[rec0:q]), (obj.dtype, numel, nbytes))
        return _StorageRef(self.buf, q, numel, obj.dtype)


# torch's storage record in one match (C speed): type name, key length + key, location length +
# location, a BININT1 / BININT2 / BININT element count, the key list repeating the key exactly
# (backreferences), the u64 count.  Length fields are verified after the match.
_RECORD_RE = re.compile(
    rb"\x80\x02\(X\x07\x00\x00\x00storageq\x00ctorch\n(\w+)\nq\x01X(.{4})([^q]*)q\x02X(.{4})([^q]*)q\x03"
    rb"(K.|M..|J.{4})Ntq\x04Q\.\x80\x02\]q\x00X\2\3q\x01a\.(.{8})", re.S)


def _parse_storage_record(mv, q):
    """The storage record torch's legacy ``_save`` writes (protocol 2) -- the persistent-id
    pickle ``('storage', torch.<T>Storage, key, location, numel, None)``, the key-list pickle
    ``[key]`` and the u64 element count -- parsed without the VM.  Returns ``(dtype, numel,
    position after the count)``, or None if ANY byte departs from that layout (the caller then
    runs the restricted VM)."""
    m = _RECORD_RE.match(mv, q)
    if m is not None:
        name, klen, key, llen, loc, nop, cnt = m.groups()
        dtype = _STORAGE_DTYPES.get(name.decode("ascii"))
        if (dtype is not None and int.from_bytes(klen, "little") == len(key)
                and int.from_bytes(llen, "little") == len(loc)):
            op = nop[0]
            numel = (nop[1] if op == 0x4B else int.from_bytes(nop[1:], "little", signed=(op == 0x4A)))
            if numel >= 0 and int.from_bytes(cnt, "little") == numel:
                return dtype, numel, m.end()
    return _parse_storage_record_slow(mv, q)


def _parse_storage_record_slow(mv, q):
    """Field-by-field form of :func:`_parse_storage_record` (LONG1 counts, keys containing
    'q', ...)."""
    n = len(mv)

    def unicode_at(p):        # BINUNICODE: 'X' u32 length, utf-8 bytes
        if p + 5 > n or mv[p] != 0x58:
            return None, p
        ln = int.from_bytes(mv[p + 1:p + 5], "little")
        if p + 5 + ln > n:
            return None, p
        return bytes(mv[p + 5:p + 5 + ln]), p + 5 + ln

    def binput(p, i):
        return p + 2 if p + 2 <= n and mv[p] == 0x71 and mv[p + 1] == i else -1

    if bytes(mv[q:q + 3]) != b"\x80\x02(":
        return None
    tag, p = unicode_at(q + 3)
    if tag != b"storage" or (p := binput(p, 0)) < 0:
        return None
    if p >= n or mv[p] != 0x63:                       # GLOBAL 'torch\n<T>Storage\n'
        return None
    e1 = bytes(mv[p + 1:p + 64]).find(b"\n")
    e2 = bytes(mv[p + 1:p + 64]).find(b"\n", e1 + 1) if e1 >= 0 else -1
    if e1 < 0 or e2 < 0 or bytes(mv[p + 1:p + 1 + e1]) != b"torch":
        return None
    dtype = _STORAGE_DTYPES.get(bytes(mv[p + 2 + e1:p + 1 + e2]).decode("ascii", "replace"))
    if dtype is None or (p := binput(p + 2 + e2, 1)) < 0:
        return None
    key, p = unicode_at(p)
    if key is None or (p := binput(p, 2)) < 0:
        return None
    loc, p = unicode_at(p)
    if loc is None or (p := binput(p, 3)) < 0 or p >= n:
        return None
    op = mv[p]
    if op == 0x4B:                                    # BININT1
        numel, p = mv[p + 1], p + 2
    elif op == 0x4D:                                  # BININT2
        numel, p = int.from_bytes(mv[p + 1:p + 3], "little"), p + 3
    elif op == 0x4A:                                  # BININT
        numel, p = int.from_bytes(mv[p + 1:p + 5], "little", signed=True), p + 5
    elif op == 0x8A:                                  # LONG1
        ln = mv[p + 1]
        numel, p = int.from_bytes(mv[p + 2:p + 2 + ln], "little", signed=True), p + 2 + ln
    else:
        return None
    if numel < 0 or bytes(mv[p:p + 2]) != b"Nt" or (p := binput(p + 2, 4)) < 0 or bytes(mv[p:p + 2]) != b"Q.":
        return None
    p += 2
    keys = b"\x80\x02]q\x00X" + len(key).to_bytes(4, "little") + key + b"q\x01a."
    if bytes(mv[p:p + len(keys)]) != keys:
        return None
    p += len(keys)
    if p + 8 > n or int.from_bytes(mv[p:p + 8], "little") != numel:
        return None
    return dtype, numel, p + 8


_STORAGE_HEADERS = []   # validated legacy-stream headers (bytes)
_STORAGE_RECORDS = {}   # record length -> {record bytes: (dtype, numel, nbytes)} (see _storage_from_span)
# The record cache is keyed by bytes the sender controls: bounded in total so no sender can grow
# host memory or the per-message lookup cost -- short records only, few distinct lengths, few
# entries (a record of another length or past the caps is simply parsed by the VM again).
RECORD_CACHE_MAX_BYTES = 512
RECORD_CACHE_MAX_LENGTHS = 8
RECORD_CACHE_MAX_ENTRIES = 4096


def _remember_record(rec: bytes, parsed) -> None:
    n = len(rec)
    if n > RECORD_CACHE_MAX_BYTES:
        return
    if n not in _STORAGE_RECORDS and len(_STORAGE_RECORDS) >= RECORD_CACHE_MAX_LENGTHS:
        return
    if sum(len(v) for v in _STORAGE_RECORDS.values()) >= RECORD_CACHE_MAX_ENTRIES:
        return
    _STORAGE_RECORDS.setdefault(n, {})[rec] = parsed


class _Span:
    __slots__ = ("start", "n")

    def __init__(self, start, n):
        self.start, self.n = start, n


_load_from_bytes_marker = object()


def _pickle_vm():
    """The C opcode loop (built in-tree by ``flame_amd.build``); ``FLAME_AMD_PICKLE_VM=py``
    selects the Python loop instead.  Missing while not opted out: an ImportError naming the
    build step, not a silent slow path."""
    if os.environ.get("FLAME_AMD_PICKLE_VM", "c") == "py":
        return None
    try:
        from . import _pickle_vm
    except ImportError as e:
        raise ImportError("flame_amd._pickle_vm is not built: run `python -m flame_amd.build` "
                          "(or set FLAME_AMD_PICKLE_VM=py)") from e
    return _pickle_vm


_VM = _pickle_vm()


def _codecs_encode(text, encoding="latin1"):
    if encoding != "latin1":
        raise pickle.UnpicklingError("only latin1-encoded bytes are allowed")
    return text.encode("latin1")


def _bytes_like(cls, *args):
    """bytes / bytearray as pickles rebuild them (``cls()``, ``cls(data[, encoding])``); never
    ``cls(n)``, which would allocate n zero bytes on the sender's say-so."""
    if args and not isinstance(args[0], (bytes, bytearray, str)):
        raise pickle.UnpicklingError(f"{cls.__name__}() from {type(args[0]).__name__} is not allowed")
    return cls(*args)


def _allow(fn):
    fn._flame_amd_allowed = True
    return fn


_CALLABLE_ALLOW = set()


@functools.lru_cache(maxsize=None)   # built once: the flame import probe is not free
def _default_globals():
    g = {
        ("torch._utils", "_rebuild_tensor_v2"): _allow(_rebuild_tensor_v2),
        ("torch.storage", "_load_from_bytes"): _load_from_bytes_marker,
        ("collections", "OrderedDict"): collections.OrderedDict,
        ("builtins", "set"): set,
        ("builtins", "frozenset"): frozenset,
        ("builtins", "bytearray"): _allow(functools.partial(_bytes_like, bytearray)),
        ("builtins", "bytes"): _allow(functools.partial(_bytes_like, bytes)),
        ("builtins", "complex"): complex,
        ("_codecs", "encode"): _allow(_codecs_encode),
    }
    for (mod, name), v in list(g.items()):     # protocols <= 2 name builtins the Python-2 way
        if mod == "builtins":
            g[("__builtin__", name)] = v
    for name, dt in _STORAGE_DTYPES.items():
        g[("torch", name)] = dt
    try:  # flame's message keys (lib/python/flame/common/constants.py MessageType)
        from flame.common.constants import MessageType  # type: ignore
        g[("flame.common.constants", "MessageType")] = MessageType
        _CALLABLE_ALLOW.add(MessageType)
    except Exception:  # noqa: BLE001
        pass
    return g


_CALLABLE_ALLOW.update({collections.OrderedDict, set, frozenset, complex})


def allow_enum(cls):
    """Allow an Enum class (by module/name) to be reconstructed from update payloads."""
    assert issubclass(cls, enum.Enum)
    _CALLABLE_ALLOW.add(cls)
    return {(cls.__module__, cls.__qualname__): cls}


def decode(payload, extra_globals: Dict[tuple, Any] = None):
    """Decode a flame update message; tensors are zero-copy views into ``payload``.

    ``payload`` must stay alive (and unmodified) while the tensors are in use;
    they are read-only views -- modifying one in place would write into the
    payload (a ``bytes`` object) without any warning.  Raises ``pickle.UnpicklingError`` for anything
    outside the allowlist (use the reference ``cloudpickle.loads`` for such
    messages).
    """
    dec = PayloadDecoder(payload, extra_globals)
    if extra_globals:
        for v in extra_globals.values():
            if isinstance(v, type) and issubclass(v, enum.Enum):
                _CALLABLE_ALLOW.add(v)
    try:
        # torch.frombuffer warns on a read-only buffer (a received `bytes` payload): the decoded
        # views are READ-ONLY by contract (see above) -- the warning is silenced for this
        # payload's decode only, once, not process-wide
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message="The given buffer is not writable", category=UserWarning)
            obj, _ = dec.load(0)
    except pickle.UnpicklingError:
        raise
    except (IndexError, KeyError, ValueError, TypeError, struct.error, UnicodeDecodeError) as e:
        raise pickle.UnpicklingError(f"malformed update payload: {type(e).__name__}: {e}") from None
    return obj


def loads(payload):
    """cloudpickle.loads drop-in for the aggregator's channel: zero-copy for update
    payloads, the reference decoder for anything the restricted VM refuses."""
    try:
        return decode(payload)
    except pickle.UnpicklingError:
        import cloudpickle  # the reference's own decoder (channel.py:321-325)
        return cloudpickle.loads(payload)


# ------------------------------------------------------------------ registered receive buffers
class RegisteredBuffer:
    """Page-lock + map a host buffer (bytearray, mmap, numpy array, shm segment) so the
    reduction kernel can read tensors decoded from it zero-copy over PCIe
    (``flame_host_register``).  Use as a context manager or call ``close()``."""

    def __init__(self, buf):
        import numpy as np
        from . import _native as N
        self.buf = buf
        self.arr = np.frombuffer(buf, dtype=np.uint8)
        self.ptr = self.arr.ctypes.data
        N.check(N.lib().flame_host_register(self.ptr, self.arr.nbytes))
        self._open = True

    def close(self):
        """Unregister after every kernel that may read the buffer has finished."""
        if self._open:
            from . import _native as N
            from . import engine
            engine._staging.drain()
            N.check(N.lib().flame_host_unregister(self.ptr))
            self._open = False
            self.arr = self.buf = None   # release the exported buffer (lets an mmap / shm close)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ------------------------------------------------------------------ LIFL shared-memory receive
class ShmReceiver:
    """Zero-copy stand-in for the LIFL SHM backend's receive (``backend/shm.py:386-391``).

    The reference opens ``SharedMemory(other + "-" + self_id)`` on every message and
    copies ``msg_size`` bytes out of it (``bytes(read_buf.buf[:msg_size])``), after
    which the channel runs ``cloudpickle.loads`` on the copy (``channel.py:321-325``).
    Here each sender's segment is opened once and (with ``register=True``, the
    default on a GPU host) page-locked and mapped for the device with
    ``flame_host_register``; :meth:`get_data` returns a memoryview of the message in
    place and :meth:`loads` decodes it with :func:`decode` -- the update's tensors are
    views into the shared segment that the reduction kernel streams over PCIe, or that
    :class:`DeviceUpdateCache` copies to HBM, without any host copy.

    Lifetime (``flame_amd.shm_lease``): the sender rewrites its segment for its next
    message (``backend/shm.py:393-403``), and nothing tells the receiver when.  So no
    consumer keeps a view past the call it was handed to: a kernel streaming the views
    zero-copy is waited for before ``do()`` returns, a FedBuff arrival queued for a
    deferred reduction and a ``DeviceUpdateCache`` entry are copied to HBM before their
    call returns, and a view used after its sender delivered a newer message raises
    instead of reading torn data.  A segment that grew is re-opened (and re-registered)
    transparently.
    """

    def __init__(self, self_id: str, register: bool = True, untrack: bool = True):
        self.self_id = self_id
        self.register = register
        self.untrack = untrack     # the writer owns (and unlinks) its segment
        self._segs = {}   # name -> (SharedMemory, RegisteredBuffer | None)

    def _segment(self, other: str, msg_size: int):
        from multiprocessing import shared_memory
        name = other + "-" + self.self_id
        seg = self._segs.get(name)
        if seg is not None and seg[0].size < msg_size:
            self._close_one(name)
            seg = None
        if seg is None:
            shm = shared_memory.SharedMemory(name)
            if self.untrack:   # python < 3.13 tracks attached segments too and unlinks them at exit
                try:
                    from multiprocessing import resource_tracker
                    resource_tracker.unregister(shm._name, "shared_memory")  # noqa: SLF001
                except Exception:  # noqa: BLE001
                    pass
            reg = RegisteredBuffer(shm.buf) if self.register else None
            seg = (shm, reg)
            self._segs[name] = seg
            import numpy as np
            from . import shm_lease
            shm_lease.add(name, np.frombuffer(shm.buf, dtype=np.uint8).ctypes.data, shm.size)
        return seg

    def get_data(self, other: str, msg_size: int) -> memoryview:
        """The message bytes in place (the reference returns a copy).  Views of the sender's
        previous message become stale (``shm_lease.check_live`` raises on them)."""
        from . import shm_lease
        shm, _ = self._segment(other, msg_size)
        shm_lease.next_generation(other + "-" + self.self_id)
        return shm.buf[:msg_size]

    def loads(self, other: str, msg_size: int):
        """get_data + zero-copy decode (falls back to cloudpickle for non-update messages);
        the message's tensors are stamped with the segment's generation."""
        from . import shm_lease
        name = other + "-" + self.self_id
        msg = loads(self.get_data(other, msg_size))
        return shm_lease.stamp(msg, name, shm_lease._gen[name])

    def _close_one(self, name):
        from . import shm_lease
        shm_lease.remove(name)
        shm, reg = self._segs.pop(name)
        if reg is not None:
            reg.close()
        del reg
        try:
            shm.close()
        except BufferError:
            pass   # views still exported; the mapping goes when they do

    def close(self):
        for name in list(self._segs):
            self._close_one(name)


# ------------------------------------------------------------------ device-resident cache
from .slab import SlotWeights  # noqa: E402  (slab imports nothing from this module)


class DeviceUpdateCache:
    """``diskcache.Cache`` stand-in that keeps received updates resident on the GPU.

    The reference aggregator pickles every update into a disk-backed cache and
    unpickles it again inside ``FedAvg.do`` (``syncfl/top_aggregator.py:93-95,156``,
    ``optimizer/fedavg.py:82``).  Here ``cache[end] = TrainResult(...)`` moves the
    update into HBM on a side stream as it arrives (overlapping the next receive):

    * ``placement="slab"`` (default): into a tiled :class:`flame_amd.slab.UpdateSlab`
      sized for ``capacity`` updates -- the layout the reduction streams at the HBM
      read ceiling; an update that does not fit (slab full or other shapes) falls
      back to ``"hbm"``;
    * ``placement="hbm"``: one device allocation per tensor (the reference's
      ``weights_to_model_device`` layout);
    * ``placement="host"``: pinned host tensors the kernel streams zero-copy.

    ``iterkeys()`` yields keys in sorted order (diskcache's ``ORDER BY key``);
    ``pop`` hands back the TrainResult with its transfer ordered before any later
    work on the caller's stream.

    ``shard=plan`` (a :class:`flame_amd.shard.ShardPlan`, e.g. ``ShardedOptimizer.plan``
    or ``ShardedHierarchy.plan``): keep only this rank's ranges of every update -- each
    arriving tensor's owned ranges are copied (strided H2D of those ranges only) into a
    slab laid out for the rank's slices, so per-GPU memory and PCIe traffic scale with
    1 / world.
    """

    def __init__(self, device=None, placement: str = "slab", capacity: int = 256, shard=None):
        if placement not in ("slab", "hbm", "host"):
            raise ValueError("placement must be 'slab', 'hbm' or 'host'")
        self.placement = placement
        self.capacity = capacity
        self.shard = shard
        self.device = torch.device(device) if device is not None else None
        self._d = collections.OrderedDict()
        self._stream = None
        self.slab = None

    def _dev(self):
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def _side_stream(self, after_current: bool = True):
        dev = self._dev()
        if self._stream is None:
            self._stream = torch.cuda.Stream(dev)
        if after_current:
            # device-resident sources may still be being produced on the caller's stream
            self._stream.wait_stream(torch.cuda.current_stream(dev))
        return self._stream

    def _fits_slab(self, w):
        from . import engine
        if any(isinstance(v, torch.Tensor) and v.dtype not in engine.DTYPE_CODE for v in w.values()):
            return False       # bool / uint8 / int8 / int16 buffers: see _put_mixed
        if self.slab is None:
            from .slab import UpdateSlab
            tmpl = self.shard.local_template() if self.shard is not None else w
            tmpl = collections.OrderedDict((k, v) for k, v in tmpl.items()
                                           if isinstance(v, torch.Tensor) and v.dtype in engine.DTYPE_CODE)
            if not tmpl:
                return False
            self.slab = UpdateSlab(tmpl, self.capacity, self._dev())
        sl = self.slab
        return (bool(sl._free) and list(w.keys()) == sl.keys
                and all(isinstance(w[k], torch.Tensor) and w[k].dtype == sl.meta[k][0]
                        and w[k].numel() == sl.meta[k][2] for k in sl.keys))

    def __setitem__(self, key, tres):
        w = getattr(tres, "weights", None)
        if isinstance(w, dict):
            from . import engine
            engine.refuse_mx([w], "DeviceUpdateCache")    # no MX slots yet: a plain cache holds MX updates
        ev = None
        shm = False
        if isinstance(w, dict) and w:
            from . import shm_lease
            for v in w.values():
                if isinstance(v, torch.Tensor) and not v.is_cuda:
                    shm_lease.check_live(v)
                    shm = shm or shm_lease.aliases(v)
        if self.shard is not None and isinstance(w, dict) and w:
            w = self.shard.slice_update(w)       # this rank's ranges only (views / host slices)
        if isinstance(w, dict) and w and self.placement in ("slab", "hbm"):
            # host-resident updates (the channel's case) need no ordering behind the caller's
            # stream, so back-to-back arrivals keep the copy engine busy while the
            # reductions of earlier arrivals run on the caller's stream
            st = self._side_stream(any(isinstance(v, torch.Tensor) and v.is_cuda for v in w.values()))
            mixed = self._split_narrow(w) if self.placement == "slab" else None
            if self.placement == "slab" and self._fits_slab(w):
                tres.weights = self.slab.put(w, stream=st)
            elif mixed is not None and self._fits_slab(mixed[0]):
                tres.weights = self._put_mixed(w, *mixed, st)
            else:
                with torch.cuda.stream(st):
                    tres.weights = w.__class__(
                        (k, v.to(self._dev(), non_blocking=True) if isinstance(v, torch.Tensor) else v)
                        for k, v in w.items())
            ev = torch.cuda.Event()
            ev.record(st)
            if shm:       # the sender may rewrite its segment once this returns: finish the copy
                ev.synchronize()
        elif isinstance(w, dict) and w and self.placement == "host" and torch.cuda.is_available():
            def pinned(v):
                if not isinstance(v, torch.Tensor) or v.is_cuda:
                    return v
                if shm:           # a view of a sender's segment: copy it out (registered = pinned)
                    return torch.empty(v.shape, dtype=v.dtype, pin_memory=True).copy_(v)
                return v if v.is_pinned() else v.pin_memory()
            tres.weights = w.__class__((k, pinned(v)) for k, v in w.items())
        if key in self._d:
            self._d.pop(key)
        self._d[key] = (tres, ev)

    @staticmethod
    def _split_narrow(w):
        """(kernel-dtype keys, bool / uint8 / int8 / int16 keys) of an update that has both."""
        from . import engine
        codes = engine.DTYPE_CODE
        if all(not isinstance(v, torch.Tensor) or v.dtype in codes for v in w.values()):
            return None                       # (the common case, checked without building dicts)
        main = collections.OrderedDict((k, v) for k, v in w.items()
                                       if isinstance(v, torch.Tensor) and v.dtype in engine.DTYPE_CODE)
        if not main or len(main) == len(w):
            return None
        return main, collections.OrderedDict((k, v) for k, v in w.items() if k not in main)

    def _put_mixed(self, w, main, extra, st):
        """The kernel-dtype keys into a slab slot, the others beside it as device tensors."""
        from .slab import MixedSlotWeights
        sw = self.slab.put(main, stream=st)
        with torch.cuda.stream(st):
            ext = {k: (v.to(self._dev(), non_blocking=True) if isinstance(v, torch.Tensor) else v)
                   for k, v in extra.items()}
        return MixedSlotWeights.of(sw, ext, list(w.keys()))

    def __getitem__(self, key):
        tres, ev = self._d[key]
        self._order(ev, tres)
        return tres

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return key in self._d

    def iterkeys(self, reverse=False):
        return iter(sorted(self._d, reverse=reverse))

    def _order(self, ev, tres):
        if ev is not None:
            from . import engine
            cur = engine.current_stream(self._dev())
            cur.wait_event(ev)
            w = tres.weights
            if isinstance(w, SlotWeights):
                return      # views of a slab slot: the slab owns the memory; the slot is recycled
                            # behind an event recorded when these views are dropped (slab.py)
            for v in w.values():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    v.record_stream(cur)

    def pop(self, key, default=None):
        if key not in self._d:
            return default
        tres, ev = self._d.pop(key)
        self._order(ev, tres)
        return tres

    def reset(self, *args, **kwargs):
        return None

    def clear(self):
        self._d.clear()
