"""Host route of MXFP4 updates (CPU only, no GPU), as tests/test_mx_host.py has it for MXFP8: every
refusal is a TypeError that names MX updates and says what is supported, raised with the aggregate
untouched and nothing launched; and engine.accumulate / reduce_ / the FedOPT and deferred rounds over
CPU tensors with the native entry points replaced by the recorders of
tests/test_engine_launch_trace.py -- one flame_agg_reduce_mxfp4 call with its code pair, chunk cursor,
scale-pointer table and byte figure."""
import collections

import numpy as np
import pytest
import torch

import scenarios as S
from flame_amd import _native as N
from flame_amd import engine, mx
from flame_amd.optimizers import optimizer_provider

from test_engine_launch_trace import CPU, STREAM
from test_uplink16_host import _calls, _segments, traced

SHAPES = collections.OrderedDict([("a", (1,)), ("b", (8193,)), ("c", (3, 5483))])       # c: 2 * 8192 + 65, odd
NUMELS = {k: int(np.prod(s)) for k, s in SHAPES.items()}
RATES = [0.5, 0.25, 0.125, 0.0625, 0.0625]
WHO = "flame_agg_reduce_mxfp4"
F4 = torch.float4_e2m1fn_x2


def _model(extra=()):
    agg = collections.OrderedDict((k, torch.full(s, 0.5)) for k, s in SHAPES.items())
    for k, dt, n in extra:
        agg[k] = torch.full((n,), 3, dtype=dt)
    return agg


def _plain(agg, i):
    return collections.OrderedDict((k, torch.full(v.shape, i + 1, dtype=v.dtype)) for k, v in agg.items())


def _updates(agg, fmt="e2m1", n=5, **kw):
    return [(mx.quantize(_plain(agg, i), fmt, **kw), RATES[i]) for i in range(n)]


def _untouched(agg):
    for k, v in agg.items():
        assert torch.equal(v, torch.full(v.shape, 0.5 if v.dtype == torch.float32 and k in SHAPES else 3, dtype=v.dtype)), k


def _refused(fn, *match):
    with traced() as tr:
        with pytest.raises(TypeError) as e:
            fn()
        assert not _calls(tr), _calls(tr)             # nothing was launched
    msg = str(e.value)
    assert "MX update" in msg and "supported" in msg and "float4_e2m1fn_x2" in msg, msg
    for m in match:
        assert m in msg, (m, msg)


def _cache(ws, counts=None):
    cache = S.SortedCache()
    for i, w in enumerate(ws):
        cache[f"e{i:02d}"] = S.TR(w, (counts or [3] * len(ws))[i], 0)
    return cache


# ---------------------------------------------------------------------------- refusals
def test_the_new_refusals_leave_the_aggregate_untouched():
    agg = _model(extra=[("nbt", torch.int64, 1)])
    acc = lambda entries, a=agg: engine.accumulate(a, entries, device=CPU)      # noqa: E731

    # an e2m1 tensor that is not 1-D
    entries = _updates(agg)
    entries[1][0]["b"] = entries[1][0]["b"].view(torch.uint8).reshape(-1, 1).view(F4)
    _refused(lambda: acc(entries), "'b'", "not 1-D")
    # not ceil(numel / 2) bytes
    entries = _updates(agg)
    entries[2][0]["c"] = entries[2][0]["c"][:-1]
    _refused(lambda: acc(entries), "'c'", f"{NUMELS['c'] // 2} bytes", f"not the {NUMELS['c'] // 2 + 1}")
    # no shapes entry
    entries = _updates(agg)
    del entries[4][0].shapes["b"]
    _refused(lambda: acc(entries), "'b'", "shapes entry")
    # a logical shape that is not the aggregate's (the same element count)
    entries = _updates(agg)
    entries[0][0].shapes["c"] = (5483, 3)
    _refused(lambda: acc(entries), "'c'", "(5483, 3)", "not the aggregate's (3, 5483)")
    # e2m1 beside a float8 format on one key: the refusal of two float8 formats
    entries = _updates(agg)
    entries[3] = (mx.quantize(_plain(agg, 3), "e4m3"), RATES[3])
    _refused(lambda: acc(entries), "two MX element formats")
    # what MXFP8 refuses, in the same words: mixtures, plain dicts, scales, the aggregate's dtype, key groups
    entries = _updates(agg)
    entries[2] = (mx.quantize(_plain(agg, 2), "e2m1", min_numel=8194), RATES[2])
    _refused(lambda: acc(entries), "'a'", "torch.float32 in others", "mixtures")
    entries = _updates(agg)
    entries[1] = (dict(entries[1][0]), RATES[1])
    _refused(lambda: acc(entries), "plain dict", "block scales")
    _refused(lambda: acc([(dict(w), r) for w, r in _updates(agg)]), "block scales")
    entries = _updates(agg)
    del entries[3][0].scales["c"]
    _refused(lambda: acc(entries), "'c'", "without scales")
    entries = _updates(agg)
    entries[0][0].scales["b"] = entries[0][0].scales["b"][:-1]
    _refused(lambda: acc(entries), "'b'", "uint8 (257,)")
    half = collections.OrderedDict((k, v.to(torch.bfloat16)) for k, v in _model().items())
    _refused(lambda: acc(_updates(_model()), half), "torch.bfloat16 aggregate")
    _refused(lambda: engine.accumulate(agg, _updates(agg), device=CPU, key_groups=[["a"], ["b", "c", "nbt"]]), "sharded wrapper")
    # reduce_: packed rows without their scales, and rows of the wrong length
    q = mx.quantize({"x": torch.ones(41)}, "e2m1")
    _refused(lambda: engine.reduce_([torch.zeros(41)], [torch.zeros(41)], [[q["x"]]], [1.0]), "without block scales")
    _refused(lambda: engine.reduce_([torch.zeros(43)], [torch.zeros(43)], [[q["x"]]], [1.0], block_scales=[[q.scales["x"]]]),
             "not an MX segment")
    with pytest.raises(TypeError, match="element dtype of an MX update"):
        engine.dtype_code(F4)
    _untouched(agg)
    # the deferred aggregate refuses at the arrival, as DeferredAggregate._check does for float8
    opt = optimizer_provider.get("fedavg", defer=True)
    bad = _updates(agg, n=1)[0][0]
    bad.shapes["c"] = (NUMELS["c"],)
    _refused(lambda: opt.do(agg, _cache([bad]), total=3), "not the aggregate's")
    _untouched(agg)


def _entries_without(entries, key):
    return [(mx.MXWeights(((k, v) for k, v in w.items() if k != key), w.scales, shapes=w.shapes), r) for w, r in entries]


def test_a_plain_uint8_key_stays_a_plain_key():
    agg = _model(extra=[("u", torch.uint8, 40)])
    entries = _updates(agg)
    assert all(w["u"].dtype == torch.uint8 and "u" not in w.scales for w, _ in entries)
    assert engine.mx_route(torch.uint8, [w for w, _ in entries], "u", (40,)) is None      # its present route
    sub = collections.OrderedDict((k, agg[k]) for k in SHAPES)          # (the uint8 key's own route needs a GPU)
    with traced() as tr:
        engine.accumulate(sub, _entries_without(entries, "u"), device=CPU)
    assert [c[0] for c in _calls(tr)] == [WHO] and _calls(tr)[0][1][4] == 3


def test_measurements_and_other_front_ends_refuse():
    agg = _model()
    ws = [w for w, _ in _updates(agg)]
    _refused(lambda: engine.update_stats(ws), "update guard", "update_stats")
    _refused(lambda: engine.update_gram(ws), "krum")
    _refused(lambda: engine.update_dist(ws, agg), "rfa")
    _refused(lambda: engine.trimmed_mean(agg, ws, 1), "trim")
    _refused(lambda: engine.selected_mean(agg, ws, 1), "trim")
    _untouched(agg)


@pytest.mark.parametrize("kwargs,what", [({"clip_threshold": 1.0}, "update guard"), ({"nonfinite": "skip"}, "update guard"),
                                          ({"trim": 1}, "trim"), ({"trim": "median"}, "trim"),
                                          ({"krum": 1}, "krum"), ({"rfa": 2}, "rfa")])
def test_fedavg_kwargs_refuse(kwargs, what):
    agg = _model()
    opt = optimizer_provider.get("fedavg", **kwargs)
    _refused(lambda: opt.do(agg, _cache([w for w, _ in _updates(agg)]), total=15), what)
    _untouched(agg)


def test_other_optimizers_slab_and_shard_refuse():
    agg = _model()
    ws = [w for w, _ in _updates(agg)]
    _refused(lambda: optimizer_provider.get("fedbuff").do(None, _cache(ws), total=15, version=1), "FedBuff")
    _refused(lambda: optimizer_provider.get("fedbuff").do(agg, _cache(ws), total=15, version=1), "FedBuff")
    _refused(lambda: optimizer_provider.get("fedbuff").do_arrivals(agg, [S.TR(w, 3, 0) for w in ws], version=1), "FedBuff")
    _refused(lambda: optimizer_provider.get("feddyn", alpha=0.01).do(agg, _cache(ws), total=15), "FedDyn")
    sc = optimizer_provider.get("scaffold", k=3)
    sc.weight_dict = {f"e{i:02d}": 1.0 for i in range(5)}
    sc.c_glob = {k: torch.zeros_like(v) for k, v in agg.items()}
    _refused(lambda: sc.do(agg, _cache(ws), total=15, control_cache=_cache([_plain(agg, i) for i in range(5)])), "SCAFFOLD")
    assert all(not v.any() for v in sc.c_glob.values())
    from flame_amd import shard
    from flame_amd.ingest import DeviceUpdateCache
    from flame_amd.slab import UpdateSlab
    slab = UpdateSlab.__new__(UpdateSlab)            # put / write refuse before they touch the slab
    _refused(lambda: slab.write(0, ws[0]), "UpdateSlab")
    with pytest.raises(TypeError, match="MX update"):
        UpdateSlab(ws[0], 2, CPU)
    for placement in ("slab", "hbm", "host"):
        cache = DeviceUpdateCache("cuda:0", placement=placement, capacity=2)
        tres = S.TR(ws[0], 3)
        _refused(lambda: cache.__setitem__("e00", tres), "DeviceUpdateCache")
        assert len(cache) == 0 and tres.weights is ws[0]
    plan = shard.ShardPlan({k: torch.empty(v.shape, device="meta") for k, v in agg.items()}, 2, 0, align=8)
    _refused(lambda: plan.local(ws[0]), "sharded wrapper")
    _refused(lambda: plan.slice_update(ws[0]), "sharded wrapper")
    _untouched(agg)


# ---------------------------------------------------------------------------- launch traces
def test_accumulate_is_one_mxfp4_launch():
    agg = _model()
    entries = _updates(agg)
    with traced() as tr:
        engine.accumulate(agg, entries, device=CPU)
    calls = _calls(tr)
    assert [c[0] for c in calls] == [WHO], calls
    a = calls[0][1]
    assert a[0] == N.FLAME_FP4_E2M1 == 12 and a[1] == N.FLAME_F32 and a[2] == 0   # the pair, no flags
    assert a[4] == 3 and a[8] == 5 and a[11] == STREAM
    assert a[10] is None                                                # scales32 NULL: the plain round
    segs = _segments(tr, a, 3)
    # numel is the logical element count; chunk_begin counts the kernel's 8,192-element chunks
    chunk = N.lib().flame_chunk_elems(N.FLAME_FP4_E2M1)
    assert chunk == 8192
    assert segs[:, 6].tolist() == list(NUMELS.values())
    assert segs[:, 7].tolist() == [0, 1, 3] and a[5] == 1 + 2 + 3
    assert segs[:, 9].tolist() == [0, 0, 0]                             # never a tiled MX row
    assert segs[:, 0].tolist() == [agg[k].data_ptr() for k in agg] == segs[:, 1].tolist()     # in place
    words = tr.blocks[a[3]["block"]].numpy()
    table = words[a[6]["off"] // 8: a[6]["off"] // 8 + 15].reshape(3, 5)
    assert table.tolist() == [[w[k].data_ptr() for w, _ in entries] for k in agg]
    assert a[7]["block"] == a[3]["block"]
    bs = words[a[7]["off"] // 8: a[7]["off"] // 8 + 15].reshape(3, 5)
    assert bs.tolist() == [[w.scales[k].data_ptr() for w, _ in entries] for k in agg]
    r32 = words[a[9]["off"] // 8:].view(np.float32)[:5]
    assert r32.tolist() == RATES
    # the recorded bytes: ceil(numel / 2) per client, one fp32 read and write per element, n scale bytes per block
    want = sum(5 * -(-n // 2) + 8 * n + 5 * -(-n // 32) for n in NUMELS.values())
    assert [e for e in tr.events if e[0] == "timed"] == [["timed", WHO, want]]


def test_one_launch_per_format_and_other_keys_keep_theirs():
    agg = _model(extra=[("nbt", torch.int64, 1), ("h", torch.bfloat16, 5)])
    entries = []
    for i in range(5):
        p = _plain(agg, i)
        lo = mx.quantize({k: p[k] for k in ("a", "b")}, "e2m1")
        hi = mx.quantize({k: p[k] for k in ("c",)}, "e5m2")
        w = mx.MXWeights(collections.OrderedDict([("a", lo["a"]), ("b", lo["b"]), ("c", hi["c"]), ("nbt", p["nbt"]),
                                                  ("h", p["h"])]), {**lo.scales, **hi.scales}, shapes=lo.shapes)
        entries.append((w, RATES[i]))
    with traced() as tr:
        engine.accumulate(agg, entries, device=CPU)
    calls = _calls(tr)
    assert sorted(c[0] for c in calls) == ["flame_agg_reduce"] * 2 + ["flame_agg_reduce_mx", WHO], calls
    by = {c[0]: c[1] for c in calls}
    assert by[WHO][0] == N.FLAME_FP4_E2M1 and by[WHO][4] == 2
    assert by["flame_agg_reduce_mx"][0] == N.FLAME_FP8_E5M2 and by["flame_agg_reduce_mx"][4] == 1
    assert not any(c[0].startswith("flame_elementwise") for c in calls)


def test_scales_take_the_scaled_instantiation():
    agg = _model(extra=[("nbt", torch.int64, 1)])
    entries = _updates(agg)
    scales = [1.0, 0.5, 1.0 / 3.0, 1e-4, 1.0]
    pre = []
    with traced(_prescaled=lambda *a: pre.append(a)) as tr:
        engine.accumulate(agg, entries, device=CPU, scales=scales)
    assert not pre                                                      # no per-entry temporaries
    calls = _calls(tr)
    assert sorted(c[0] for c in calls) == ["flame_agg_reduce", WHO]
    a = [c[1] for c in calls if c[0] == WHO][0]
    assert isinstance(a[10], dict) and a[10]["block"] == a[3]["block"]  # scales32 non-NULL, inside the block
    s32 = tr.blocks[a[3]["block"]].numpy()[a[10]["off"] // 8:].view(np.float32)[:5]
    assert s32.tolist() == [float(np.float32(s)) for s in scales]


def test_reduce_groups_by_format_and_refuses_flags():
    q4 = mx.quantize({"x": torch.ones(9), "y": torch.ones(7)}, "e2m1")
    q8 = mx.quantize({"x": torch.ones(4099)}, "e4m3")
    outs = [torch.zeros(9), torch.zeros(4099), torch.zeros(7), torch.zeros(5)]
    cl = [[q4["x"]] * 2, [q8["x"]] * 2, [q4["y"]] * 2, [torch.ones(5)] * 2]
    bs = [[q4.scales["x"]] * 2, [q8.scales["x"]] * 2, [q4.scales["y"]] * 2, None]
    with traced() as tr:
        engine.reduce_(outs, outs, cl, [0.5, 0.5], block_scales=bs)
    calls = _calls(tr)
    assert sorted((c[0], c[1][0], c[1][1]) for c in calls[:2]) == [("flame_agg_reduce_mx", N.FLAME_FP8_E4M3, N.FLAME_F32),
                                                                   (WHO, N.FLAME_FP4_E2M1, N.FLAME_F32)]
    assert calls[2][0] == "flame_agg_reduce" and len(calls) == 3
    a = [c[1] for c in calls if c[0] == WHO][0]
    assert a[4] == 2 and _segments(tr, a, 2)[:, 6].tolist() == [9, 7]
    with traced() as tr:
        with pytest.raises(NotImplementedError, match="init_first"):
            engine.reduce_(outs[:1], None, cl[:1], [0.5, 0.5], init_first=True, block_scales=bs[:1])
        with pytest.raises(NotImplementedError, match="seg_rates"):
            engine.reduce_(outs[:1], outs[:1], cl[:1], None, seg_rates=[[0.5, 0.5]], block_scales=bs[:1])
        with pytest.raises(TypeError, match="MX"):
            engine.reduce_([torch.zeros(9, dtype=torch.float64)], [torch.zeros(9, dtype=torch.float64)], cl[:1], [0.5, 0.5],
                           block_scales=bs[:1])
        assert not _calls(tr)


def test_xcd_map_by_chunk_count():
    agg = _model()
    with traced(XCD_MAP_MIN_CHUNKS=2) as tr:
        engine.accumulate(agg, _updates(agg), device=CPU)
    assert _calls(tr)[0][1][2] == N.FLAME_AGG_XCD_MAP


@pytest.mark.parametrize("sort", ["fedadam", "fedyogi", "fedadagrad"])
def test_fedopt_round_is_two_launches(sort):
    """Past the passthrough round: the MXFP4 reduction, then flame_fedopt_reduce_adapt with no clients."""
    agg = _model()
    opt = optimizer_provider.get(sort)
    opt.current_weights = collections.OrderedDict((k, torch.zeros_like(v)) for k, v in agg.items())
    with traced(pick_device=lambda *a: CPU) as tr:
        opt.do(agg, _cache([w for w, _ in _updates(agg)]), total=15)
    calls = _calls(tr)
    assert [c[0] for c in calls] == [WHO, "flame_fedopt_reduce_adapt"], [c[0] for c in calls]
    assert calls[0][1][4] == 3 and calls[0][1][8] == 5
    assert calls[1][1][7] == 0                                          # the adaptive step reads no clients
    # the eager chain's queue sends MX arrivals to the per-call path
    opt = optimizer_provider.get(sort, defer=True)
    opt.current_weights = collections.OrderedDict((k, torch.zeros_like(v)) for k, v in agg.items())
    with traced(pick_device=lambda *a: CPU) as tr:
        opt.do(agg, _cache([w for w, _ in _updates(agg, n=1)]), total=3)
    assert [c[0] for c in _calls(tr)] == [WHO, "flame_fedopt_reduce_adapt"]


def test_deferred_fedavg_flushes_into_one_launch():
    agg = _model()
    opt = optimizer_provider.get("fedavg", defer=True)
    ws = [w for w, _ in _updates(agg, n=3)]
    cache = S.SortedCache()
    with traced(pick_device=lambda *a: CPU) as tr:
        for i, w in enumerate(ws):
            cache[f"e{i:02d}"] = S.TR(w, 3, 0)
            out = opt.do(agg, cache, total=3 * (i + 1))
        assert not _calls(tr)                                           # queued: nothing launched yet
        out["a"]                                                        # the first read flushes
    calls = _calls(tr)
    assert [c[0] for c in calls] == [WHO] and calls[0][1][8] == 3 and calls[0][1][4] == 3
