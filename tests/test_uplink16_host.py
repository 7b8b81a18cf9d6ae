"""Host route of bf16 / f16 updates into an fp32 aggregate (CPU only, no GPU): engine.accumulate and
engine.reduce_ over CPU tensors with the native entry points, the metadata upload and the stream
lookups replaced by the recorders of tests/test_engine_launch_trace.py.  What is pinned: which
entry point each key reaches, how often, with which dtype pair, chunk cursor, scale pointer and
byte figure."""
import collections
import contextlib

import numpy as np
import pytest
import torch

from flame_amd import _native as N
from flame_amd import engine

from test_engine_launch_trace import CPU, STREAM, Tracer, _Event, _Stream, _Timings, _patched

T = 2048
NUMELS = collections.OrderedDict([("a", 1), ("b", 2049), ("c", 3 * 2048 + 17)])
RATES = [0.5, 0.25, 0.125, 0.0625, 0.0625]
CODE = {torch.bfloat16: N.FLAME_BF16, torch.float16: N.FLAME_F16}


@contextlib.contextmanager
def traced(**extra):
    tr = Tracer()
    stream = _Stream()
    with contextlib.ExitStack() as st:
        st.enter_context(_patched(N, lib=lambda: tr))
        st.enter_context(_patched(engine._staging, upload=tr.upload, hold=lambda t, device: None))
        st.enter_context(_patched(engine, _stream_ptr=lambda device: STREAM, current_stream=lambda device: stream,
                                  host_device_pointer=lambda p: p, kernel_events=_Timings(tr),
                                  _require_hip=lambda device, who: None, ARGMETA=False, **extra))
        st.enter_context(_patched(torch.cuda, Event=_Event))
        yield tr


def _model(extra=()):
    agg = collections.OrderedDict((k, torch.zeros(n, dtype=torch.float32)) for k, n in NUMELS.items())
    for k, dt, n in extra:
        agg[k] = torch.zeros(n, dtype=dt)
    return agg


def _updates(agg, dt, n=5, other=None):
    other = other or {}
    return [({k: torch.ones(v.shape, dtype=other.get(k, dt if v.dtype == torch.float32 else v.dtype)) for k, v in agg.items()},
             RATES[i]) for i in range(n)]


def _calls(tr, prefix=""):
    return [(e[1], e[2]) for e in tr.events if e[0] == "call" and e[1].startswith(prefix)]


def _segments(tr, call_args, n_segs):
    blk = tr.blocks[call_args[3]["block"]]
    return blk.numpy()[:n_segs * engine.SEG_WORDS].reshape(n_segs, engine.SEG_WORDS)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_accumulate_is_one_mixed_launch(dt):
    agg = _model()
    entries = _updates(agg, dt)
    with traced() as tr:
        engine.accumulate(agg, entries, device=CPU)
    calls = _calls(tr)
    assert [c[0] for c in calls] == ["flame_agg_reduce_mixed"], calls
    a = calls[0][1]
    assert a[0] == CODE[dt] and a[1] == N.FLAME_F32 and a[2] == 0       # the pair, no flags
    assert a[4] == 3 and a[7] == 5 and a[10] == STREAM
    assert a[9] is None                                                 # scales32 NULL: the plain round
    segs = _segments(tr, a, 3)
    # chunk_begin counts 2,048-element chunks of the CLIENT dtype (fp32's own chunk is 1,024)
    assert segs[:, 6].tolist() == list(NUMELS.values())
    assert segs[:, 7].tolist() == [0, 1, 3] and a[5] == 1 + 2 + 4
    assert segs[:, 0].tolist() == [agg[k].data_ptr() for k in agg] == segs[:, 1].tolist()     # in place
    table = tr.blocks[a[3]["block"]].numpy()[a[6]["off"] // 8: a[6]["off"] // 8 + 15].reshape(3, 5)
    assert table.tolist() == [[w[k].data_ptr() for w, _ in entries] for k in agg]
    r32 = tr.blocks[a[3]["block"]].numpy()[a[8]["off"] // 8:].view(np.float32)[:5]
    assert r32.tolist() == RATES
    # the recorded bytes: n 16-bit reads, one fp32 read, one fp32 write per element
    timed = [e for e in tr.events if e[0] == "timed"]
    assert timed == [["timed", "flame_agg_reduce_mixed", sum(NUMELS.values()) * (5 * 2 + 8)]]


def test_other_keys_keep_their_launches():
    agg = _model(extra=[("f", torch.float32, 33), ("nbt", torch.int64, 1), ("h", torch.bfloat16, 5)])
    entries = _updates(agg, torch.bfloat16, other={"f": torch.float32})
    with traced() as tr:
        engine.accumulate(agg, entries, device=CPU)
    names = [c[0] for c in _calls(tr)]
    assert sorted(names) == ["flame_agg_reduce"] * 3 + ["flame_agg_reduce_mixed"], names
    assert not any(n.startswith("flame_elementwise") for n in names)
    by = {c[1][0]: c[1] for c in _calls(tr, "flame_agg_reduce") if c[0] == "flame_agg_reduce"}
    assert sorted(by) == sorted([N.FLAME_F32, N.FLAME_I64, N.FLAME_BF16])     # one launch per same-dtype group
    assert by[N.FLAME_F32][3] == 1 and by[N.FLAME_I64][3] == 1 and by[N.FLAME_BF16][3] == 1
    mixed = [c[1] for c in _calls(tr) if c[0] == "flame_agg_reduce_mixed"][0]
    assert mixed[4] == 3 and _segments(tr, mixed, 3)[:, 6].tolist() == list(NUMELS.values())


def test_key_of_two_update_dtypes_stays_on_the_old_route():
    agg = _model()
    entries = _updates(agg, torch.bfloat16)
    entries[2][0]["b"] = entries[2][0]["b"].to(torch.float32)        # one entry holds b as fp32
    entries[4][0]["c"] = entries[4][0]["c"].to(torch.float16)        # one entry holds c as f16, the others bf16
    seen = []
    with traced(_accumulate_mixed=lambda agg_, keys, sub, device: seen.append(list(keys))) as tr:
        engine.accumulate(agg, entries, device=CPU)
    assert seen == [["b", "c"]]
    calls = _calls(tr)
    assert [c[0] for c in calls] == ["flame_agg_reduce_mixed"] and calls[0][1][4] == 1
    assert _segments(tr, calls[0][1], 1)[0, 0] == agg["a"].data_ptr()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_scales_take_the_scaled_instantiation(dt):
    agg = _model(extra=[("nbt", torch.int64, 1)])
    entries = _updates(agg, dt)
    scales = [1.0, 0.5, 1.0 / 3.0, 1e-4, 1.0]
    pre = []
    with traced(_prescaled=lambda *a: pre.append(a)) as tr:
        engine.accumulate(agg, entries, device=CPU, scales=scales)
    assert not pre                                                      # no per-entry temporaries
    calls = _calls(tr)
    assert sorted(c[0] for c in calls) == ["flame_agg_reduce", "flame_agg_reduce_mixed"]
    a = [c[1] for c in calls if c[0] == "flame_agg_reduce_mixed"][0]
    assert isinstance(a[9], dict) and a[9]["block"] == a[3]["block"]    # scales32 non-NULL, inside the block
    s32 = tr.blocks[a[3]["block"]].numpy()[a[9]["off"] // 8:].view(np.float32)[:5]
    assert s32.tolist() == [float(np.float32(s)) for s in scales]
    # the integer key is never scaled
    i64 = [c[1] for c in calls if c[0] == "flame_agg_reduce"][0]
    assert i64[0] == N.FLAME_I64


def test_reduce_groups_by_both_dtypes_and_refuses_flags():
    outs = [torch.zeros(9), torch.zeros(4099), torch.zeros(7), torch.zeros(5)]
    cl = [[torch.ones(9, dtype=torch.bfloat16)] * 2, [torch.ones(4099, dtype=torch.float16)] * 2,
          [torch.ones(7, dtype=torch.bfloat16)] * 2, [torch.ones(5)] * 2]
    with traced() as tr:
        engine.reduce_(outs, outs, cl, [0.5, 0.5])
    calls = _calls(tr)
    assert [(c[0], c[1][0], c[1][1]) for c in calls[:2]] == [("flame_agg_reduce_mixed", N.FLAME_BF16, N.FLAME_F32),
                                                             ("flame_agg_reduce_mixed", N.FLAME_F16, N.FLAME_F32)]
    assert calls[0][1][4] == 2 and calls[1][1][4] == 1 and calls[2][0] == "flame_agg_reduce" and len(calls) == 3
    with traced() as tr:
        with pytest.raises(NotImplementedError, match="init_first"):
            engine.reduce_(outs[:1], None, cl[:1], [0.5, 0.5], init_first=True)
        with pytest.raises(NotImplementedError, match="seg_rates"):
            engine.reduce_(outs[:1], outs[:1], cl[:1], None, seg_rates=[[0.5, 0.5]])
        # clients that differ among themselves keep the old error
        with pytest.raises(NotImplementedError, match="differs from aggregate dtype"):
            engine.reduce_(outs[:1], outs[:1], [[cl[0][0], cl[0][0].to(torch.float16)]], [0.5, 0.5])
        with pytest.raises(NotImplementedError, match="differs from aggregate dtype"):
            engine.reduce_([torch.zeros(9, dtype=torch.float64)], [torch.zeros(9, dtype=torch.float64)], cl[:1], [0.5, 0.5])
        assert not _calls(tr)


def test_xcd_map_for_rows_only():
    agg = _model()
    entries = _updates(agg, torch.bfloat16)
    with traced(XCD_MAP_MIN_CHUNKS=2) as tr:
        engine.accumulate(agg, entries, device=CPU)
    assert _calls(tr)[0][1][2] == N.FLAME_AGG_XCD_MAP
