"""Host-side launch trace of flame_amd.engine's launchers (CPU only, no GPU).

The launch functions are otherwise reached by GPU tests only.  Here each one runs over CPU
tensors, or over bare ``Seg`` / ``HierSeg`` / ``DynSeg`` pointer integers, with the native
library's launch entry points, the metadata upload and the stream lookups replaced by recorders.
A case's trace is the ordered list of

* ``["upload", <block hex>]``          every ``engine._staging.upload``, with the block's bytes,
* ``["call", <entry point>, [args]]``  every native call, with every argument,
* ``["timed", <name>, <bytes>]``       every timing record,
* ``["reduce_", [outs], [[clients]], [rates], {kwargs}]``  a nested ``engine.reduce_`` (``trimmed_mean``
  sends its integer keys there through ``accumulate``), by label: ``reduce_`` has a device check of
  its own, and what it launches is pinned by the ``reduce_*`` cases,
* ``["return", [[shape, dtype, <hex>], ...]]``  the arrays a measuring front end returns,
* ``["raise", <type>, <message>, <flame_partial>]``  the exception a case ends in.

Addresses are position-independent: an argument equal to ``data_ptr()`` of a tensor the case
labelled is that label; a pointer into an uploaded block is ``{"block": i, "off": n}``; a host
block handed to a kernel-argument entry point is ``{"argmeta": <hex>}``; inside a block, a word
equal to a labelled tensor's address is replaced by a fixed stand-in for that label.  What the
engine allocates itself is named by its place in the entry point's arguments: an output pointer is
``{"out": <byte offset from the case's first output pointer>}``, the scratch buffer ``"scratch"``.

The expected traces are ``tests/golden/engine_launch_trace.json``, written by
``tests/golden/make_engine_launch_trace.py`` from the engine as it stood before its launch paths
were merged into one (the ``update_stats`` / ``update_gram`` / ``trimmed_mean`` cases: before those
three were given one front end); the comparison is event by event, byte by byte.
"""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from flame_amd import _native as N
from flame_amd import engine

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launch_trace.json")
CPU = torch.device("cpu")
STREAM = 0x5157
FORWARDED = ("flame_chunk_elems", "flame_scale_add_chunk_elems", "flame_agg_argmeta_max_bytes",
             "flame_update_stats_scratch_bytes", "flame_update_gram_scratch_bytes", "flame_update_gram_max_clients",
             "flame_agg_trimmed_max_k")
# position of (host block, its byte count) in the kernel-argument entry points
ARGMETA_AT = {"flame_agg_reduce_argmeta": 2, "flame_fedopt_reduce_adapt_argmeta": 3, "flame_hier_fedbuff_argmeta": 2}
# position of (the output pointers, the scratch pointer) in the entry points whose caller allocates both
SELF_ALLOCATED = {"flame_update_stats": ((6, 7), 8), "flame_update_gram": ((6, 7), 8)}


class _Event:
    def __init__(self, *a, **kw):
        pass

    def record(self, *a):
        pass


class _Stream:
    def wait_event(self, ev):
        pass


class Tracer:
    """The recorders of one case."""

    def __init__(self, fail_at=None, rc=N.FLAME_EHIP):
        self.events = []
        self.labels = {}          # data_ptr -> (label, stand-in address)
        self.blocks = []          # uploaded blocks (CPU tensors, kept alive: no address is reused)
        self.tensors = []
        self.fail_at, self.rc, self.n_calls = fail_at, rc, 0
        self.out_base = None      # the first output pointer an entry point of SELF_ALLOCATED was handed
        self.real = N.lib()

    def t(self, label, tensor):
        """Register a tensor of the case under ``label``."""
        assert tensor.data_ptr() not in self.labels and tensor.data_ptr() % engine.VEC_BYTES == 0
        self.labels[tensor.data_ptr()] = (label, (len(self.labels) + 1) << 36)
        self.tensors.append(tensor)
        return tensor

    def _hex(self, raw: bytes) -> str:
        words = np.frombuffer(raw, dtype=np.uint64).copy()
        for ptr, (_, stand_in) in self.labels.items():
            words[words == np.uint64(ptr)] = np.uint64(stand_in)
        return words.tobytes().hex()

    def _arg(self, a):
        if isinstance(a, (int, np.integer)) and not isinstance(a, bool):
            a = int(a)
            if a in self.labels:
                return self.labels[a][0]
            for i, b in enumerate(self.blocks):
                if b.data_ptr() <= a <= b.data_ptr() + b.numel() * b.element_size():
                    return {"block": i, "off": a - b.data_ptr()}
            return a
        if a is None or isinstance(a, float):
            return a
        raise TypeError(f"untraceable argument {a!r}")

    # ---- the seams
    def upload(self, meta, device):
        assert device == CPU and meta.dtype == np.int64
        dev = torch.from_numpy(meta.copy())
        self.blocks.append(dev)
        self.events.append(["upload", self._hex(meta.tobytes())])
        return dev

    def __getattr__(self, name):            # stands in for the ctypes library
        if not name.startswith("flame_"):
            raise AttributeError(name)
        if name in FORWARDED:
            return getattr(self.real, name)

        def call(*args):
            if name == "flame_last_error":
                self.events.append(["call", name, []])
                return b"recorded failure"
            args = list(args)
            at = ARGMETA_AT.get(name)
            if at is not None:
                args[at] = {"argmeta": self._hex(ctypes.string_at(args[at], args[at + 1]))}
            outs, scratch = SELF_ALLOCATED.get(name, ((), None))
            for i in outs:
                if self.out_base is None:
                    self.out_base = args[i]
                args[i] = {"out": args[i] - self.out_base}
            if scratch is not None:
                args[scratch] = "scratch"
            self.events.append(["call", name, [a if isinstance(a, (dict, str)) else self._arg(a) for a in args]])
            self.n_calls += 1
            return self.rc if self.n_calls == self.fail_at else 0
        return call

    def timed(self, ev):
        self.events.append(["timed", ev[0], int(ev[3])])

    def reduce_(self, outs, ins, clients, rates, **kw):
        assert ins is outs
        name = lambda t: self.labels[t.data_ptr()][0]     # noqa: E731
        self.events.append(["reduce_", [name(o) for o in outs], [[name(c) for c in row] for row in clients],
                            [float(r).hex() for r in rates], {k: v for k, v in kw.items() if v is not None}])

    def returned(self, arrays):
        self.events.append(["return", [[list(a.shape), str(a.dtype), a.tobytes().hex()] for a in arrays]])


class _Timings(list):
    def __init__(self, tracer):
        super().__init__()
        self.tracer = tracer

    def append(self, ev):
        self.tracer.timed(ev)


@contextlib.contextmanager
def _patched(obj, **attrs):
    missing = object()
    old = {k: obj.__dict__.get(k, missing) for k in attrs}
    for k, v in attrs.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is missing:
                delattr(obj, k)
            else:
                setattr(obj, k, v)


def run_case(name):
    """The trace of case ``name`` (a list of JSON-able events)."""
    fn, opts = CASES[name]
    tr = Tracer(fail_at=opts.get("fail_at"))
    stream = _Stream()
    with contextlib.ExitStack() as st:
        st.enter_context(_patched(N, lib=lambda: tr))
        st.enter_context(_patched(engine._staging, upload=tr.upload, hold=lambda t, device: None))
        st.enter_context(_patched(engine, _stream_ptr=lambda device: STREAM, current_stream=lambda device: stream,
                                  host_device_pointer=lambda p: p, kernel_events=_Timings(tr),
                                  _hip_device=lambda device, who, *dicts, prefer=None: CPU,
                                  ARGMETA=opts.get("argmeta", True),
                                  XCD_MAP_MIN_CHUNKS=opts.get("xcd", engine.XCD_MAP_MIN_CHUNKS)))
        st.enter_context(_patched(torch.cuda, Event=_Event))
        try:
            out = fn(tr)
            if out is not None:
                tr.returned(out)
        except Exception as e:  # noqa: BLE001 - the exception is part of the trace
            tr.events.append(["raise", type(e).__name__, str(e), bool(getattr(e, "flame_partial", False))])
    return json.loads(json.dumps(tr.events))


# ------------------------------------------------------------------ cases
CASES = {}


def case(name, **opts):
    def deco(fn):
        CASES[name] = (fn, opts)
        return fn
    return deco


def P(i):
    """A bare, 16-byte-aligned stand-in address."""
    return 0x7000_0000 + i * 0x10_0000


def _reduce_segs(n_clients=3, tile_stride=0, init_first=False, numels=(1, 1025)):
    return [engine.Seg(n, out=P(10 * s), inp=0 if init_first else P(10 * s + 1),
                       clients=[P(100 * (s + 1) + c) for c in range(n_clients)], tile_stride=tile_stride if s else 0)
            for s, n in enumerate(numels)]


RATES3 = [0.5, 0.3, 0.2]


def _launch_reduce(tr, code=N.FLAME_F32, **kw):
    segs = kw.pop("segs", None) or _reduce_segs(init_first=kw.get("init_first", False))
    rates = kw.pop("rates", RATES3)
    keep = []
    engine._launch_reduce(code, segs, rates, CPU, keep, **kw)
    assert len(keep) == len(tr.blocks) and all(a is b for a, b in zip(keep, tr.blocks))


case("reduce_f32_argmeta")(_launch_reduce)
case("reduce_f32_table", argmeta=False)(_launch_reduce)
case("reduce_f32_table_xcd", argmeta=False, xcd=2)(_launch_reduce)
case("reduce_f32_argmeta_xcd", xcd=2)(_launch_reduce)
case("reduce_f32_table_xcd_tiled", argmeta=False, xcd=2)(
    lambda tr: _launch_reduce(tr, segs=_reduce_segs(tile_stride=8192)))
case("reduce_f32_init_first")(lambda tr: _launch_reduce(tr, init_first=True))
case("reduce_f32_init_first_table", argmeta=False)(lambda tr: _launch_reduce(tr, init_first=True))
case("reduce_f32_seg_rates")(
    lambda tr: _launch_reduce(tr, rates=[RATES3, [0.125, 0.25, 0.625]], seg_rates=True))
case("reduce_f32_seg_rates_table", argmeta=False)(
    lambda tr: _launch_reduce(tr, rates=[RATES3, [0.125, 0.25, 0.625]], seg_rates=True))
case("reduce_f64_argmeta")(lambda tr: _launch_reduce(tr, code=N.FLAME_F64))
case("reduce_f64_table", argmeta=False)(lambda tr: _launch_reduce(tr, code=N.FLAME_F64))
case("reduce_bf16_argmeta")(lambda tr: _launch_reduce(tr, code=N.FLAME_BF16))
case("reduce_i64_argmeta")(lambda tr: _launch_reduce(tr, code=N.FLAME_I64))
case("reduce_i64_table", argmeta=False)(lambda tr: _launch_reduce(tr, code=N.FLAME_I64))
case("reduce_f32_600_clients")(
    lambda tr: _launch_reduce(tr, segs=_reduce_segs(600, numels=(1025,)), rates=[(i % 7 + 1) / 4096 for i in range(600)]))
case("reduce_scaled_f32")(lambda tr: _launch_reduce(tr, scales=[1.0, 0.7, 0.1]))
case("reduce_scaled_f64")(lambda tr: _launch_reduce(tr, code=N.FLAME_F64, scales=[1.0, 0.7, 0.1]))
case("reduce_scaled_f32_xcd", xcd=2)(lambda tr: _launch_reduce(tr, scales=[1.0, 0.7, 0.1]))
case("reduce_scaled_f32_xcd_tiled", xcd=2)(
    lambda tr: _launch_reduce(tr, segs=_reduce_segs(tile_stride=8192), scales=[1.0, 0.7, 0.1]))
case("reduce_scaled_seg_rates_raises")(
    lambda tr: _launch_reduce(tr, rates=[RATES3, RATES3], seg_rates=True, scales=[1.0, 0.7, 0.1]))
case("reduce_scaled_i64_raises")(lambda tr: _launch_reduce(tr, code=N.FLAME_I64, scales=[1.0, 0.7, 0.1]))


# ---- FedOPT: CPU tensors
FEDOPT_KEYS = [("f32", torch.float32, 1025), ("bf16", torch.bfloat16, 7), ("f64", torch.float64, 3)]


def _fedopt_tensors(tr, keys, n_clients, roles):
    out = {r: [tr.t(f"{r}.{nm}", torch.zeros(n, dtype=dt)) for nm, dt, n in keys] for r in roles}
    out["clients"] = [[tr.t(f"client{c}.{nm}", torch.zeros(n, dtype=dt)) for c in range(n_clients)]
                      for nm, dt, n in keys]
    return out


def _fedopt_reduce_adapt(tr, state_zero, variant="fedadam"):
    t = _fedopt_tensors(tr, FEDOPT_KEYS, 2, ("avg", "base", "cur", "cur_out", "m", "v"))
    t["avg"][2] = None                   # the f64 key writes no average
    t["cur"][1] = None                   # the bf16 key's current IS its average
    engine.fedopt_reduce_adapt_(variant, t["avg"], t["base"], t["cur"], t["cur_out"], t["m"], t["v"], t["clients"],
                                [0.75, 0.25], engine.fedopt_scalars(0.9, 0.99, 0.1, 1e-3), state_zero,
                                cur_is_avg=[False, True, False])


case("fedopt_adapt_state_zero")(lambda tr: _fedopt_reduce_adapt(tr, True))
case("fedopt_adapt")(lambda tr: _fedopt_reduce_adapt(tr, False, "fedyogi"))
case("fedopt_adapt_state_zero_table", argmeta=False)(lambda tr: _fedopt_reduce_adapt(tr, True, "fedadagrad"))
case("fedopt_adapt_table", argmeta=False)(lambda tr: _fedopt_reduce_adapt(tr, False))
case("fedopt_adapt_fail_second", fail_at=2)(lambda tr: _fedopt_reduce_adapt(tr, False))


@case("fedopt_adapt_f64_needs_raw_scalars")
def _fedopt_adapt_plain_tuple(tr):
    # the f32 key comes first: the missing doubles must raise before ITS launch
    t = _fedopt_tensors(tr, FEDOPT_KEYS[0::2], 1, ("avg", "base", "cur", "cur_out", "m", "v"))
    engine.fedopt_reduce_adapt_("fedadam", t["avg"], t["base"], t["cur"], t["cur_out"], t["m"], t["v"], t["clients"],
                                [1.0], tuple(engine.fedopt_scalars(0.9, 0.99, 0.1, 1e-3)), False)


CHAIN_KEYS = [("f32", torch.float32, 1025), ("f16", torch.float16, 7), ("f64", torch.float64, 3)]


def _fedopt_chain(tr, state_zero=False, step_end=(0, 1, 1), keys=CHAIN_KEYS, hyper=None):
    t = _fedopt_tensors(tr, keys, len(step_end), ("base", "cur", "cur_out", "m", "v"))
    aliased = [True, False, True][:len(keys)]
    for s, a in enumerate(aliased):
        if a:
            t["cur"][s] = None
    engine.fedopt_chain_("fedyogi", t["base"], t["cur"], t["cur_out"], t["m"], t["v"], t["clients"],
                         [0.5, 0.25, 0.25][:len(step_end)], list(step_end),
                         hyper or engine.fedopt_scalars(0.9, 0.99, 0.1, 1e-3), state_zero, aliased)


case("fedopt_chain")(_fedopt_chain)
case("fedopt_chain_state_zero", argmeta=False)(lambda tr: _fedopt_chain(tr, True))
case("fedopt_chain_fail_first", fail_at=1)(_fedopt_chain)
case("fedopt_chain_fail_second", fail_at=2)(_fedopt_chain)
case("fedopt_chain_open_last_step")(lambda tr: _fedopt_chain(tr, step_end=(1, 1, 0)))
case("fedopt_chain_f64_needs_raw_scalars")(
    lambda tr: _fedopt_chain(tr, hyper=tuple(engine.fedopt_scalars(0.9, 0.99, 0.1, 1e-3))))
case("fedopt_chain_int64")(
    lambda tr: _fedopt_chain(tr, keys=[("f32", torch.float32, 5), ("i64", torch.int64, 5)]))


# ---- FedBuff scale_add: CPU tensors
def _scale_add(tr, with_delta, base_dt=torch.float32, agg_numel=1025):
    bases = [tr.t("base0", torch.zeros(1025, dtype=base_dt)), tr.t("base1", torch.zeros(3, dtype=base_dt))]
    aggs = [tr.t("agg0", torch.zeros(agg_numel, dtype=base_dt)), tr.t("agg1", torch.zeros(3, dtype=base_dt))]
    deltas = [tr.t("delta0", torch.zeros(1025, dtype=base_dt)), tr.t("delta1", torch.zeros(3, dtype=base_dt))]
    engine.scale_add_(bases, aggs, 5, deltas if with_delta else None)


case("scale_add")(lambda tr: _scale_add(tr, False))
case("scale_add_delta")(lambda tr: _scale_add(tr, True))
case("scale_add_bf16_delta")(lambda tr: _scale_add(tr, True, torch.bfloat16))
case("scale_add_numel_mismatch")(lambda tr: _scale_add(tr, False, agg_numel=1024))
case("scale_add_int64_base")(lambda tr: _scale_add(tr, False, torch.int64))


# ---- the co-located hierarchy: bare pointers
def _hier(tr, M=2, C=2, with_delta=False, code=N.FLAME_F32, top=True, **kw):
    segs = [engine.HierSeg(numel=n, mid_w=[P(1000 * (s + 1) + m) for m in range(M)],
                           clients=np.asarray([P(2000 * (s + 1) + i) for i in range(M * C)], dtype=np.uint64),
                           mid_delta=[P(1000 * (s + 1) + 500 + m) for m in range(M)] if with_delta else None,
                           top_w=P(s + 1) if kw.get("top_goal") is not None else 0,
                           top_in=P(20 + s) if kw.get("top_accum") else 0, top_out=P(20 + s) if top else 0,
                           tile_stride=4096 if s and kw.get("mid_readonly") else 0,
                           mid_tile_stride=8192 if s and kw.get("sync") else 0)
            for s, n in enumerate((1, 1025))]
    kw.setdefault("top_accum", False)
    kw.setdefault("top_goal", None)
    keep = []
    engine.hier_fedbuff_(segs, code, [[(m + c + 1) / 16 for c in range(C)] for m in range(M)], [2 + m for m in range(M)],
                         [1 / (m + 1) for m in range(M)], device=CPU, keep=keep, **kw)
    assert len(keep) == len(tr.blocks) and all(a is b for a, b in zip(keep, tr.blocks))


case("hier")(_hier)
case("hier_delta")(lambda tr: _hier(tr, with_delta=True))
case("hier_delta_table", argmeta=False)(lambda tr: _hier(tr, with_delta=True))
case("hier_table", argmeta=False)(_hier)
case("hier_top_goal")(lambda tr: _hier(tr, top_accum=True, top_goal=3))
case("hier_sync")(lambda tr: _hier(tr, top_accum=True, sync=True, with_delta=True))
case("hier_mid_readonly_bf16")(lambda tr: _hier(tr, code=N.FLAME_BF16, top_accum=True, mid_readonly=True))
case("hier_one_middle_no_top")(lambda tr: _hier(tr, M=1, C=3, with_delta=True, top=False))
case("hier_40x20")(lambda tr: _hier(tr, M=40, C=20, top_accum=True, top_goal=3, with_delta=True))


# ---- FedDyn: bare pointers
def _feddyn(tr, arrivals, dict_order, had, code=N.FLAME_F32):
    steps, n_phase1 = engine.feddyn_program(arrivals, dict_order, had)
    ends = {e: i for i, e in enumerate(dict_order)}
    segs = [engine.DynSeg(n, out=P(10 * s), inp=P(10 * s), cld=P(10 * s + 1),
                          steps=[(P(100 * (s + 1) + ends[e]) if f & N.FLAME_DYN_W else 0,
                                  P(200 * (s + 1) + ends[e]) if f & N.FLAME_DYN_HIN else 0,
                                  P(200 * (s + 1) + ends[e]) if f & N.FLAME_DYN_HOUT else 0) for f, e in steps],
                          tile_stride=4096 * s, hist_tile_stride=8192 * s)
            for s, n in enumerate((1, 1025))]
    keep = []
    engine.feddyn_round_(code, segs, [f for f, _ in steps], n_phase1, 0.5, 1 / len(dict_order), CPU, keep)
    assert len(keep) == len(tr.blocks) and all(a is b for a, b in zip(keep, tr.blocks))


case("feddyn_merged")(lambda tr: _feddyn(tr, ["a", "b"], ["a", "b", "c"], {"a", "c"}))
case("feddyn_two_phase")(lambda tr: _feddyn(tr, ["b", "a"], ["a", "b"], {"a"}, N.FLAME_F64))


# ---- the launches that read updates and write no model: CPU tensors
MEASURED_KEYS = [("a", torch.float32, 1), ("b", torch.float32, 1025), ("h", torch.bfloat16, 7), ("nbt", torch.int64, 1)]


def _updates(tr, n, keys=MEASURED_KEYS, lacking=()):
    """``n`` updates over ``keys``; ``lacking``: (update index, key name) pairs left out."""
    return [{nm: tr.t(f"u{i}.{nm}", torch.zeros(numel, dtype=dt)) for nm, dt, numel in keys if (i, nm) not in lacking}
            for i in range(n)]


def _tiny(n, dt=torch.float32):
    """``n`` one-element updates (unlabelled: a case that raises before it reads them)."""
    return [{"w": torch.zeros(1, dtype=dt)} for _ in range(n)]


INT_KEY = [("nbt", torch.int64, 1)]

case("update_stats")(lambda tr: engine.update_stats(_updates(tr, 3), device=CPU))
case("update_stats_ragged")(lambda tr: engine.update_stats(_updates(tr, 3, lacking=[(1, "b")]), device=CPU))
case("update_stats_f64")(lambda tr: engine.update_stats(_updates(tr, 2, [("d", torch.float64, 3)]), device=CPU))
case("update_stats_no_float_key")(lambda tr: engine.update_stats(_updates(tr, 3, INT_KEY), device=CPU))
case("update_stats_no_updates")(lambda tr: engine.update_stats([], device=CPU))

case("update_gram")(lambda tr: engine.update_gram(_updates(tr, 3), device=CPU))
case("update_gram_missing_key")(lambda tr: engine.update_gram(_updates(tr, 3, lacking=[(1, "b")]), device=CPU))
case("update_gram_dtype_mismatch")(
    lambda tr: engine.update_gram(_updates(tr, 2) + [{nm: torch.zeros(numel, dtype=torch.float16 if nm == "h" else dt)
                                                      for nm, dt, numel in MEASURED_KEYS}], device=CPU))
case("update_gram_shape_mismatch")(
    lambda tr: engine.update_gram(_updates(tr, 2) + [{nm: torch.zeros(numel + (nm == "a"), dtype=dt)
                                                      for nm, dt, numel in MEASURED_KEYS}], device=CPU))
case("update_gram_over_capacity")(lambda tr: engine.update_gram(_tiny(1025), device=CPU))
case("update_gram_no_float_key")(lambda tr: engine.update_gram(_updates(tr, 3, INT_KEY), device=CPU))
case("update_gram_no_updates")(lambda tr: engine.update_gram([], device=CPU))

TRIMMED_KEYS = [("a", torch.float32, 1), ("b", torch.float32, 1025), ("h", torch.float16, 7), ("nbt", torch.int64, 1)]


def _trimmed(tr, n=5, k=2, keys=TRIMMED_KEYS, agg_keys=None, **kw):
    agg = {nm: tr.t(f"agg.{nm}", torch.zeros(numel, dtype=dt)) for nm, dt, numel in agg_keys or keys}
    with _patched(engine, reduce_=tr.reduce_):
        engine.trimmed_mean(agg, _updates(tr, n, keys), k, device=CPU, **kw)


case("trimmed_mean")(_trimmed)
case("trimmed_mean_init_first")(lambda tr: _trimmed(tr, keys=TRIMMED_KEYS[:3], init_first=True))
case("trimmed_mean_init_first_int_key")(lambda tr: _trimmed(tr, init_first=True))
case("trimmed_mean_xcd", xcd=2)(_trimmed)
case("trimmed_mean_k_over_capacity")(
    lambda tr: engine.trimmed_mean({"w": torch.zeros(1)}, _tiny(2 * engine.trimmed_max_k() + 3),
                                   engine.trimmed_max_k() + 1, device=CPU))
case("trimmed_mean_too_few_updates")(lambda tr: _trimmed(tr, n=4))
case("trimmed_mean_wrong_key_set")(lambda tr: _trimmed(tr, keys=TRIMMED_KEYS[1:], agg_keys=TRIMMED_KEYS))


# ------------------------------------------------------------------ the test
def _expected():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_the_cases():
    assert sorted(_expected()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name):
    got, exp = run_case(name), _expected()[name]
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, f"{name}: event {i} differs"
    assert len(got) == len(exp), f"{name}: {len(got)} events, expected {len(exp)}"


def _calls(trace):
    return [e for e in trace if e[0] == "call"]


def test_chain_uploads_every_group_before_the_first_launch():
    kinds = [e[0] for e in run_case("fedopt_chain")]
    assert kinds == ["upload"] * 3 + ["call", "timed"] * 3


def test_chain_partial_flag_only_after_a_launch_ran():
    assert run_case("fedopt_chain_fail_first")[-1][0::3] == ["raise", False]
    assert run_case("fedopt_chain_fail_second")[-1][0::3] == ["raise", True]


def test_tau_is_rounded_per_dtype():
    f32, bf16, f64 = _calls(run_case("fedopt_adapt"))
    assert f32[1] == bf16[1] == "flame_fedopt_reduce_adapt_argmeta" and f64[1] == "flame_fedopt_reduce_adapt_f64"
    assert f32[2][-2] == float(np.float32(1e-3))
    assert bf16[2][-2] == float(torch.tensor(float(np.float32(1e-3)), dtype=torch.bfloat16)) != f32[2][-2]
    assert f64[2][-7:-1] == [0.9, 1 - 0.9, 0.99, 1 - 0.99, 0.1, 1e-3]


def test_xcd_map_only_on_untiled_tables():
    flag = {n: _calls(run_case(n))[0][2][1] & N.FLAME_AGG_XCD_MAP for n in CASES if n.startswith("reduce_")
            and not n.endswith("raises")}
    assert {n for n, f in flag.items() if f} == {"reduce_f32_table_xcd", "reduce_scaled_f32_xcd"}


def test_measuring_front_ends_share_one_output_block_and_one_scratch():
    """Slot 0 first; a second client set's sums behind the first's, the counts behind all sums."""
    for name, want in (("update_stats", [[0, 24]] * 2), ("update_stats_ragged", [[0, 40], [24, 64], [0, 40]]),
                       ("update_gram", [[0, 72]] * 2)):
        calls = _calls(run_case(name))
        assert [[a["out"] for a in c[2][6:8]] for c in calls] == want and all(c[2][8] == "scratch" for c in calls)
    assert [e[0] for e in run_case("update_stats_no_float_key")] == ["return"]
    assert [e[0] for e in run_case("update_gram_no_updates")] == ["return"]


def test_trimmed_mean_counter_goes_last_with_equal_rates():
    trace = run_case("trimmed_mean")
    assert [e[1] for e in _calls(trace)] == ["flame_agg_trimmed"] * 2 and trace[-1][0] == "reduce_"
    assert trace[-1][1:] == [["agg.nbt"], [[f"u{i}.nbt" for i in range(5)]], [(1.0 / 5).hex()] * 5, {}]
    flags = {n: [c[2][1] for c in _calls(run_case(n))] for n in ("trimmed_mean", "trimmed_mean_init_first",
                                                               "trimmed_mean_xcd")}
    assert flags == {"trimmed_mean": [0, 0], "trimmed_mean_init_first": [N.FLAME_AGG_INIT_FIRST] * 2,
                     "trimmed_mean_xcd": [N.FLAME_AGG_XCD_MAP, 0]}


def test_raising_cases_upload_nothing():
    for n in ("reduce_scaled_seg_rates_raises", "reduce_scaled_i64_raises", "fedopt_chain_int64",
              "fedopt_chain_open_last_step", "scale_add_int64_base", "scale_add_numel_mismatch",
              "fedopt_adapt_f64_needs_raw_scalars", "fedopt_chain_f64_needs_raw_scalars",
              "update_gram_missing_key", "update_gram_dtype_mismatch", "update_gram_shape_mismatch",
              "update_gram_over_capacity", "trimmed_mean_init_first_int_key", "trimmed_mean_k_over_capacity",
              "trimmed_mean_too_few_updates", "trimmed_mean_wrong_key_set"):
        trace = run_case(n)
        assert [e[0] for e in trace] == ["raise"], n
