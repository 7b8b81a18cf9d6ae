"""GPU: bf16 / f16 updates into an fp32 model in one reduction launch (flame_agg_reduce_mixed).

* ``engine.reduce_`` bitwise against the torch-CPU restatement of the reference's two statements
  (``tmp = v * rate; base += tmp``, tests/uplink16_case.py): sizes around the lane vector and the
  2,048-element chunk, client counts around the unroll of 8, contiguous tensors, tiled slab slots,
  views one element off alignment (clients and base separately), several segments per launch.
* All 65,536 bit patterns of each 16-bit dtype under eight rates and six bases.
* Clip scales against the restatement; all-ones scales against the unscaled launch.
* The route the parent commit took (``engine._accumulate_promoted``) gives the same bits.
* Through the classes: ``DeviceUpdateCache`` + ``FedAvg.do`` against tests/golden/uplink16.npz with
  the launch accounting, a clipped round, a deferred flush, three rounds of each FedOPT sort.
* One case on a non-default stream with late inputs (tests/stream_case.py).
"""
from collections import OrderedDict

import pytest
import torch

import scenarios as S
import stream_case as SC
import uplink16_case as U

pytestmark = [pytest.mark.gpu]
oracle = pytest.mark.oracle

DEV = "cuda:0"
CDTS = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
NUMELS = [1, 7, 8, 9, 2047, 2048, 2049, 3 * 2048 + 17]
NCL = [1, 7, 8, 9, 17]


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()
    torch.empty(1, device=DEV)


def make_amd(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


class Launches:
    """Names of the native launches made inside the block (engine._recorders)."""

    def __enter__(self):
        from flame_amd import engine
        self.events = []
        engine._recorders.append(self.events)
        return self

    def __exit__(self, *exc):
        from flame_amd import engine
        engine._recorders.remove(self.events)
        self.names = [ev[0] for ev in self.events]
        self.bytes = {ev[0]: ev[3] for ev in self.events}
        return False

    def count(self, name):
        return sum(1 for n in self.names if n == name)

    def elementwise(self):
        return sum(1 for n in self.names if n.startswith("flame_elementwise"))


# ---------------------------------------------------------------------------- shapes
_DATA = {}


def _data(cdt):
    """Per numel: the fp32 base, 17 client tensors, the rates; the restated result for every client
    count of NCL.  Built once per dtype and never written."""
    if cdt not in _DATA:
        g = torch.Generator().manual_seed(160 + CDTS.index(cdt))
        rates = (torch.rand(max(NCL), generator=g, dtype=torch.float64) / 8).tolist()
        base = [torch.randn(n, generator=g) for n in NUMELS]
        cl = [[(torch.randn(n, generator=g) * (0.1 + i)).to(cdt) for i in range(max(NCL))] for n in NUMELS]
        exp = {nc: [U.restate(b, c[:nc], rates[:nc]) for b, c in zip(base, cl)] for nc in NCL}
        _DATA[cdt] = (base, cl, rates, exp)
    return _DATA[cdt]


def _off_by_one(t):
    """A device view of ``t``'s values that starts one element past a fresh allocation."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:]
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize("layout", ["contiguous", "slab", "client_misaligned", "base_misaligned"])
@pytest.mark.parametrize("cdt", CDTS, ids=IDS)
def test_reduce_shapes(cdt, layout):
    """Every numel as one segment of ONE launch per client count."""
    from flame_amd import engine
    from flame_amd.slab import UpdateSlab
    base, cl, rates, exp = _data(cdt)
    keys = [f"k{n}" for n in NUMELS]
    for nc in NCL:
        if layout == "base_misaligned":
            outs = [_off_by_one(b) for b in base]
        else:
            outs = [b.to(DEV, copy=True) for b in base]
        if layout == "slab":
            slab = UpdateSlab(OrderedDict((k, c[0]) for k, c in zip(keys, cl)), nc, DEV)
            slots = [slab.put(OrderedDict((k, c[i].to(DEV)) for k, c in zip(keys, cl))) for i in range(nc)]
            rows = [[sw[k] for sw in slots] for k in keys]
            assert all(engine.tiled_stride(r[0], n) for r, n in zip(rows, NUMELS))
        elif layout == "client_misaligned":
            rows = [[_off_by_one(c[i]) for i in range(nc)] for c in cl]
        else:
            rows = [[c[i].to(DEV) for i in range(nc)] for c in cl]
        with Launches() as ln:
            engine.reduce_(outs, outs, rows, rates[:nc])
        torch.cuda.synchronize()
        assert ln.names == ["flame_agg_reduce_mixed"], ln.names
        assert ln.bytes["flame_agg_reduce_mixed"] == sum(NUMELS) * (nc * 2 + 8)
        S.same_bits(f"{layout}/n={nc}", dict(zip(keys, outs)), dict(zip(keys, exp[nc])))


# ---------------------------------------------------------------------------- every 16-bit operand
RATES = [1.0, 1.0 / 3.0, 0.75, 1e-3, 3.0, -0.5, 0.0, 2.0 ** -20]
BASES = [0.0, -0.0, 1.0, -1e-30, 3e38, float("inf")]


@pytest.mark.parametrize("cdt", CDTS, ids=IDS)
def test_every_16bit_value(cdt):
    """All 65,536 bit patterns as ``v``, three clients holding permutations of them; one launch per
    rate triple (every rate is the first client's once), one segment per base.  Bitwise, signed zeros
    included; a NaN equals a NaN.  Covers f16 overflow to inf under rate 3.0 and both dtypes'
    subnormals."""
    from flame_amd import engine
    g = torch.Generator().manual_seed(5)
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)      # wraps: every pattern once
    vs = [bits.view(cdt)] + [bits[torch.randperm(65536, generator=g)].view(cdt) for _ in range(2)]
    dev_vs = [v.to(DEV) for v in vs]
    keys = [f"base{j}" for j in range(len(BASES))]
    for i in range(len(RATES)):
        rates = [RATES[i], RATES[(i + 1) % 8], RATES[(i + 3) % 8]]
        outs = [torch.full((65536,), b, dtype=torch.float32, device=DEV) for b in BASES]
        engine.reduce_(outs, outs, [dev_vs] * len(BASES), rates)
        torch.cuda.synchronize()
        exp = [U.restate(torch.full((65536,), b, dtype=torch.float32), vs, rates) for b in BASES]
        S.same_bits(f"rates={rates}", dict(zip(keys, outs)), dict(zip(keys, exp)))


# ---------------------------------------------------------------------------- scaled
@pytest.mark.parametrize("layout", ["contiguous", "slab"])
@pytest.mark.parametrize("cdt", CDTS, ids=IDS)
def test_scaled(cdt, layout):
    from flame_amd import engine
    from flame_amd.slab import UpdateSlab
    base, cl, rates, exp = _data(cdt)
    keys = [f"k{n}" for n in NUMELS]
    nc = 9
    scales = [[1.0, 0.5, 1.0 / 3.0, 1e-4][i % 4] for i in range(nc)]
    if layout == "slab":
        slab = UpdateSlab(OrderedDict((k, c[0]) for k, c in zip(keys, cl)), nc, DEV)
        slots = [slab.put(OrderedDict((k, c[i].to(DEV)) for k, c in zip(keys, cl))) for i in range(nc)]
        rows = [[sw[k] for sw in slots] for k in keys]
    else:
        rows = [[c[i].to(DEV) for i in range(nc)] for c in cl]
    outs = [b.to(DEV, copy=True) for b in base]
    with Launches() as ln:
        engine.reduce_(outs, outs, rows, rates[:nc], scales=scales)
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_mixed"], ln.names
    want = [U.restate(b, c[:nc], rates[:nc], scales) for b, c in zip(base, cl)]
    S.same_bits(f"scaled/{layout}", dict(zip(keys, outs)), dict(zip(keys, want)))
    # all-ones scales: the scaled instantiation gives the plain launch's bits
    ones = [b.to(DEV, copy=True) for b in base]
    engine.reduce_(ones, ones, rows, rates[:nc], scales=[1.0] * nc)
    torch.cuda.synchronize()
    S.same_bits(f"ones/{layout}", dict(zip(keys, ones)), dict(zip(keys, exp[nc])))


# ---------------------------------------------------------------------------- the parent's route
@pytest.mark.parametrize("layout", ["contiguous", "slab"])
@pytest.mark.parametrize("cdt", CDTS, ids=IDS)
def test_promoted_route_gives_the_same_bits(cdt, layout):
    """``engine._accumulate_promoted`` (per client one temporary in the update's dtype and one in
    fp32, then a rate-1 reduction) is what the parent commit ran for these keys: the same bits."""
    from flame_amd import engine
    from flame_amd.slab import UpdateSlab
    base, cl, rates, exp = _data(cdt)
    keys = [f"k{n}" for n in NUMELS]
    nc = 9
    ups = [OrderedDict((k, c[i].to(DEV)) for k, c in zip(keys, cl)) for i in range(nc)]
    if layout == "slab":
        slab = UpdateSlab(ups[0], nc, DEV)
        ups = [slab.put(u) for u in ups]
    entries = list(zip(ups, rates[:nc]))
    old = OrderedDict((k, b.to(DEV, copy=True)) for k, b in zip(keys, base))
    for k in keys:
        engine._accumulate_promoted(old, k, entries, torch.device(DEV))
    new = OrderedDict((k, b.to(DEV, copy=True)) for k, b in zip(keys, base))
    with Launches() as ln:
        engine.accumulate(new, entries)
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_mixed"], ln.names
    S.same_bits(f"old/{layout}", old, dict(zip(keys, exp[nc])))
    S.same_bits(f"new/{layout}", new, S.to_cpu(old))


# ---------------------------------------------------------------------------- through the classes
def _host_cache(capacity=16):
    from flame_amd.ingest import DeviceUpdateCache
    return DeviceUpdateCache(DEV, placement="slab", capacity=capacity)


@oracle
def test_fedavg_from_the_device_cache(golden):
    """Host bf16 updates through DeviceUpdateCache(placement="slab") and FedAvg.do: the reference's
    result (uplink16.npz ``model/``) bit for bit, one flame_agg_reduce_mixed for the two bf16 keys,
    one flame_agg_reduce each for the fp32-update key and the int64 counter, no interpreter launch."""
    fx = golden("uplink16.npz")
    m = fx.meta["model"]
    cache = _host_cache()
    for i, (e, c) in enumerate(zip(m["end_ids"], m["counts"])):
        cache[e] = S.TR(OrderedDict(fx.weights(f"model/client{i}")), c)
    assert cache.slab is not None and cache.slab.meta["w1"][0] == torch.bfloat16
    base = S.to_dev(fx.weights("model/base"), DEV)
    opt = make_amd("fedavg")
    with Launches() as ln:
        out = opt.do(base, cache, total=m["total"], num_trainers=m["n"])
    torch.cuda.synchronize()
    assert out is base and len(cache) == 0
    assert ln.count("flame_agg_reduce_mixed") == 1 and ln.count("flame_agg_reduce") == 2, ln.names
    assert ln.elementwise() == 0 and len(ln.names) == 3, ln.names
    assert ln.bytes["flame_agg_reduce_mixed"] == (2049 + 77) * (9 * 2 + 8)
    S.assert_bitwise("model", out, fx.weights("model/out"))
    by_id = {e: (fx.weights(f"model/client{i}"), c) for i, (e, c) in enumerate(zip(m["end_ids"], m["counts"]))}
    b0 = fx.weights("model/base")
    want = {k: U.restate(b0[k], [by_id[e][0][k] for e in m["order"]], [by_id[e][1] / m["total"] for e in m["order"]])
            for k in b0}
    S.assert_bitwise("model/restated", out, want)


@oracle
@pytest.mark.parametrize("layout", ["tensors", "cache"])
def test_fedavg_fixture(golden, layout):
    """uplink16.npz ``fedavg/``: bf16 keys and f16 keys of 77 / 2,048 / 4,099 elements, 9 clients --
    one launch per client dtype, bitwise the reference."""
    fx = golden("uplink16.npz")
    cache = _host_cache()

    def wrap(w, i):
        return S.to_dev(w, DEV) if layout == "tensors" else OrderedDict(w)
    if layout == "cache":
        m = fx.meta["fedavg"]
        for i, (e, c) in enumerate(zip(m["end_ids"], m["counts"])):
            cache[e] = S.TR(OrderedDict(fx.weights(f"fedavg/client{i}")), c)
        base = S.to_dev(fx.weights("fedavg/base"), DEV)
        with Launches() as ln:
            out = make_amd("fedavg").do(base, cache, total=m["total"], num_trainers=m["n"])
        res = [("fedavg/out", out, fx.weights("fedavg/out"))]
    else:
        with Launches() as ln:
            res = U.run_fedavg(fx, "fedavg", make_amd, DEV, wrap)
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_mixed"] * 2, ln.names
    for label, got, exp in res:
        S.assert_bitwise(f"{layout}:{label}", got, exp)


def _model_round(g, n=9):
    base = OrderedDict([("w1", torch.randn(2049, generator=g)), ("w2", torch.randn(3, 2048 + 5, generator=g)),
                        ("f", torch.randn(33, generator=g)), ("nbt", torch.tensor(7))])
    ups = [OrderedDict([("w1", (torch.randn(2049, generator=g) * 0.02 * (i + 1)).to(torch.bfloat16)),
                        ("w2", (torch.randn(3, 2048 + 5, generator=g) * 0.02 * (i + 1)).to(torch.bfloat16)),
                        ("f", torch.randn(33, generator=g) * 0.02), ("nbt", torch.tensor(i))]) for i in range(n)]
    return base, ups, [5 + 3 * i for i in range(n)]


def _restate_model(base, ups, rates, scales=None):
    out = OrderedDict()
    for k, b in base.items():
        sc = scales if (scales is not None and b.is_floating_point()) else None
        out[k] = U.restate(b, [u[k] for u in ups], rates, sc)
    return out


@pytest.mark.parametrize("layout", ["tensors", "cache"])
def test_fedavg_clipped(layout):
    """FedAvg(clip_threshold=...): the clipped updates' scales ride into the same launch
    (``scales32``), no per-entry temporaries; bitwise the restatement with the recorded scales."""
    base, ups, counts = _model_round(torch.Generator().manual_seed(31))
    total = sum(counts)
    opt = make_amd("fedavg", clip_threshold=3.0)
    if layout == "cache":
        cache = _host_cache()
        for i, (u, c) in enumerate(zip(ups, counts)):
            cache[f"e{i:02d}"] = S.TR(OrderedDict((k, v.clone()) for k, v in u.items()), c)
    else:
        cache = S.SortedCache()
        for i, (u, c) in enumerate(zip(ups, counts)):
            cache[f"e{i:02d}"] = S.TR(S.to_dev(u, DEV), c)
    dev_base = S.to_dev(base, DEV)
    with Launches() as ln:
        out = opt.do(dev_base, cache, total=total)
    torch.cuda.synchronize()
    scales = [r.scale for r in opt.update_stats]
    assert any(s < 1.0 for s in scales) and any(s == 1.0 for s in scales), scales
    assert ln.count("flame_agg_reduce_mixed") == 1 and ln.elementwise() == 0, ln.names
    assert ln.count("flame_agg_reduce_scaled") == 1 and ln.count("flame_agg_reduce") == 1, ln.names      # f, nbt
    S.same_bits(f"clipped/{layout}", out, _restate_model(base, ups, [c / total for c in counts], scales))


def test_fedavg_deferred_flush():
    """FedAvg(defer=True): eager arrivals queued, one flush when the result is read."""
    base, ups, counts = _model_round(torch.Generator().manual_seed(32), n=6)
    opt = make_amd("fedavg", defer=True)
    dev_base = S.to_dev(base, DEV)
    cache = S.SortedCache()
    want, running, out = base, 0, None
    for i, (u, c) in enumerate(zip(ups, counts)):
        running += c
        cache[f"e{i:02d}"] = S.TR(S.to_dev(u, DEV), c)
        out = opt.do(dev_base, cache, total=running)
        want = _restate_model(want, [u], [c / running])
    with Launches() as ln:
        got = OrderedDict((k, out[k]) for k in out)        # the read runs the queue
    torch.cuda.synchronize()
    assert ln.count("flame_agg_reduce_mixed") == 1 and ln.elementwise() == 0, ln.names
    S.same_bits("deferred", got, want)


@oracle
@pytest.mark.parametrize("sort", U.SORTS)
def test_fedopt_rounds(golden, sort):
    """Three rounds with bf16 updates into the fp32 model: the contract of the fp32 FedOPT fixtures --
    SURVEY §8(c) against the reference's torch-CPU run (uplink16.npz), bitwise against the C oracle
    with the correctly rounded root.  The keys are fused (no interpreter launch), m_t / v_t fp32."""
    from oracle import oracle as O
    fx = golden("uplink16.npz")

    def each_round(r, opt):
        if opt.m_t is not None:
            assert all(t.dtype == torch.float32 and t.is_cuda for t in list(opt.m_t.values()) + list(opt.v_t.values()))

    with Launches() as ln:
        got = U.run_fedopt(fx, sort, make_amd, DEV, each_round=each_round)
    names = ln.names
    assert ln.elementwise() == 0, names
    assert ln.count("flame_agg_reduce_mixed") == 3 and ln.count("flame_fedopt_reduce_adapt") == 2, names
    U.check_fedopt(sort, got)
    ora = U.run_fedopt(fx, sort, lambda s, **kw: O.OracleFedOPT(s, sqrt_rn=True, **kw), "cpu")
    assert [l for l, _, _ in got] == [l for l, _, _ in ora]
    for (label, g, _), (_, o, _) in zip(got, ora):
        S.same_bits(f"{sort}:{label} vs the C oracle", g, o)


# ---------------------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def delay():
    d = SC.Delay()
    yield d
    d.free()


def test_round_on_a_late_stream(delay):
    """One FedAvg round of bf16 updates with every input poisoned until late on a stream of its own:
    asynchronous, bitwise the restatement and the default-stream run."""
    base0, ups, counts = _model_round(torch.Generator().manual_seed(33), n=7)
    total = sum(counts)
    want = _restate_model(base0, ups, [c / total for c in counts])

    def case(L):
        opt = make_amd("fedavg")
        base, srcs = L.weights(base0), [L.weights(u) for u in ups]
        cache = S.SortedCache()
        for i, (u, c) in enumerate(zip(srcs, counts)):
            cache[f"e{i:02d}"] = S.TR(OrderedDict(u), c)
        with L.stream():
            L.start()
            with L.call("uplink16/fedavg"):
                out = opt.do(base, cache, total=total)
            L.reuse(*srcs)
            res = {"out": L.snap(out)}
        L.finish()
        S.same_bits("late", res["out"], want)
        return res
    ready = case(SC.Late(delay, ready=True))
    late = case(SC.Late(delay))
    SC.assert_same("uplink16", ready, late)
