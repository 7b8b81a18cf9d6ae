"""The ``rfa`` / ``rfa_nu`` kwargs' host side, without a GPU: validation
(``flame_amd/optimizer/rfa.py``), every refused combination with the cache still full, the classes
that do not take the kwarg, the stage's iteration against tests/rfa_ref.py, the all-beta-zero stop,
an empty eligible set, the records and metrics, and that the defaults run none of the new code.
``engine.update_stats`` / ``update_dist`` / ``reduce_`` are replaced by CPU statements and
``engine.accumulate`` by a recorder."""
import json
import math

import numpy as np
import pytest
import torch

import rfa_ref as R
import scenarios as S


def _opt(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


class CountingCache(S.SortedCache):
    """A cache double that counts pops."""

    def __init__(self):
        super().__init__()
        self.pops = []

    def pop(self, k, default=None):
        self.pops.append(k)
        return super().pop(k, default)


def _cache(ups, counts=None):
    c = CountingCache()
    for i, u in enumerate(ups):
        c[f"e{i:02d}"] = S.TR(u, 1 if counts is None else counts[i])
    return c


def _ups(n, numel=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(numel, generator=g)
    return [{"w": mu + 0.1 * torch.randn(numel, generator=g), "nbt": torch.tensor(3 + i)} for i in range(n)]


SORTS = (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5}),
         ("fedadam", {}), ("fedyogi", {}), ("fedadagrad", {}))


@pytest.fixture
def cpu_engine(monkeypatch):
    """The engine's measurements and the centre's reduction as CPU statements; records the calls."""
    from flame_amd import engine
    calls = {"stats": [], "dist": [], "accumulate": [], "reduce": []}

    def update_stats(ws, device=None):
        ws = list(ws)
        calls["stats"].append(len(ws))
        zero = {k: torch.zeros_like(v) for w in ws for k, v in w.items() if v.is_floating_point()}
        d2, bad = R.dist2(ws, zero)
        return np.asarray(d2, np.float64), np.asarray(bad, np.int64)

    def update_dist(ws, center, device=None):
        ws = list(ws)
        calls["dist"].append((len(ws), {k: v.clone() for k, v in center.items()}))
        d2, bad = calls["dist_override"](ws, center) if "dist_override" in calls else R.dist2(ws, center)
        return np.asarray(d2, np.float64), np.asarray(bad, np.int64)

    def reduce_(outs, ins, clients, rates, *, init_first=False, **kw):
        assert init_first and ins is None
        calls["reduce"].append(list(rates))
        for o, row in zip(outs, clients):
            acc = None
            for c, r in zip(row, rates):
                tmp = (c * np.float32(r).item()).to(o.dtype)
                acc = tmp if acc is None else acc + tmp
            o.copy_(acc)

    def accumulate(agg, entries, **kw):
        calls["accumulate"].append(([r for _, r in entries], kw.get("scales")))

    monkeypatch.setattr(engine, "update_stats", update_stats)
    monkeypatch.setattr(engine, "update_dist", update_dist)
    monkeypatch.setattr(engine, "reduce_", reduce_)
    monkeypatch.setattr(engine, "accumulate", accumulate)
    monkeypatch.setattr(engine, "_hip_device", lambda device, who, *d, **k: torch.device("cpu"))
    return calls


def test_kwarg_validation():
    from flame_amd.optimizer import rfa
    assert rfa.check_kwargs(None, None) == (None, None)
    assert rfa.check_kwargs(1, None) == (1, 1e-6) and rfa.check_kwargs(7, 0.5) == (7, 0.5)
    assert rfa.check_kwargs(3, 1) == (3, 1.0)
    for bad in (True, False):
        with pytest.raises(TypeError, match="bool"):
            _opt("fedavg", rfa=bad)
        with pytest.raises(TypeError, match="rfa_nu"):
            _opt("fedavg", rfa=3, rfa_nu=bad)
    for bad in (1.0, 2.5, "3", [3], (3,), {"T": 3}, 1 + 0j, float("nan")):
        with pytest.raises(TypeError, match="rfa"):
            _opt("fedavg", rfa=bad)
    for bad in (0, -1, -50):
        with pytest.raises(ValueError, match="rfa"):
            _opt("fedavg", rfa=bad)
    for bad in (0, 0.0, -1e-6, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="rfa_nu"):
            _opt("fedavg", rfa=3, rfa_nu=bad)
    for bad in ("1e-6", [1e-6], 1e-6 + 0j):
        with pytest.raises(TypeError, match="rfa_nu"):
            _opt("fedavg", rfa=3, rfa_nu=bad)
    with pytest.raises(ValueError, match="needs rfa"):
        _opt("fedavg", rfa_nu=1e-6)
    for sort, kw in SORTS:
        o = _opt(sort, rfa=4, rfa_nu=1e-3, **kw)
        assert o.rfa == 4 and o.rfa_nu == 1e-3 and o.rfa_records == [] and o.rfa_trace == []
        assert _opt(sort, rfa=2, **kw).rfa_nu == 1e-6
        d = _opt(sort, **kw)
        assert d.rfa is None and d.rfa_nu is None
    with pytest.raises(TypeError):
        _opt("fedavg", False, 256, 1 << 30, None, "keep", None, None, None, 3)      # keyword-only


@pytest.mark.parametrize("other,match", [({"trim": 1}, "choose trim or rfa"), ({"krum": 1}, "choose krum or rfa"),
                                         ({"clip_threshold": 1.0}, "per-client scale"),
                                         ({"defer": True}, "other updates")])
def test_every_refusal_row(other, match):
    from flame_amd.optimizers import optimizer_provider as P
    for sort, kw in SORTS:
        if "trim" in other and sort in ("fedadam", "fedyogi", "fedadagrad"):
            continue                                    # the FedOPT family refuses trim itself, first
        if "defer" in other and sort in ("fedprox", "fedgft"):
            continue                                    # these take no defer
        with pytest.raises(NotImplementedError, match=match) as e:
            P.get(sort, rfa=3, **other, **kw)
        assert "geometric-median" in str(e.value)
    # a bad value is a bad value before it is refused
    with pytest.raises(ValueError):
        P.get("fedavg", rfa=0, **other)
    with pytest.raises(TypeError):
        P.get("fedavg", rfa=2.0, **other)
    # nonfinite= alone is allowed
    assert P.get("fedavg", rfa=3, nonfinite="skip").guarded


def test_the_wrapper_and_key_groups_refusals_leave_the_cache_full(cpu_engine):
    from flame_amd.optimizers import optimizer_provider as P
    from flame_amd.shard import ShardedOptimizer
    with pytest.raises(NotImplementedError, match="all-reduce of n doubles"):
        ShardedOptimizer(P.get("fedavg", rfa=2))
    with pytest.raises(NotImplementedError, match="geometric-median"):
        ShardedOptimizer(P.get("fedadam", rfa=1))
    for sort in ("fedavg", "fedadam"):
        opt = P.get(sort, rfa=2)
        cache = _cache(_ups(5))
        with pytest.raises(NotImplementedError, match="all-reduce of n doubles"):
            opt.do({"w": torch.zeros(40), "nbt": torch.tensor(0)}, cache, total=5, flame_amd_key_groups=[["w"], ["nbt"]])
        assert cache.pops == [] and len(cache) == 5
        assert cpu_engine["stats"] == [] and cpu_engine["accumulate"] == [] and opt.rfa_records == []


def test_classes_that_do_not_take_the_kwarg():
    from flame_amd.optimizers import optimizer_provider as P
    for sort, kw in (("fedbuff", {}), ("feddyn", {"alpha": 0.1}), ("scaffold", {"k": 3})):
        with pytest.raises(TypeError, match="rfa"):
            P.get(sort, rfa=3, **kw)
        with pytest.raises(TypeError, match="rfa_nu"):
            P.get(sort, rfa_nu=1e-6, **kw)


def test_defaults_run_no_new_code(monkeypatch):
    from flame_amd import engine
    from flame_amd.optimizer import rfa

    def boom(*a, **k):
        raise AssertionError("called")
    monkeypatch.setattr(engine, "update_dist", boom)
    monkeypatch.setattr(rfa, "iterate", boom)
    monkeypatch.setattr(rfa, "centre", boom)
    seen = []
    monkeypatch.setattr(engine, "accumulate", lambda agg, entries, **kw: seen.append([r for _, r in entries]))
    for sort, kw in SORTS[:3]:
        opt = _opt(sort, **kw)
        assert opt.rfa is None and opt.rfa_nu is None
        opt.do({"w": torch.zeros(3)}, _cache([{"w": torch.ones(3)}, {"w": torch.ones(3)}], [1, 3]), total=4)
        assert seen[-1] == [0.25, 0.75] and opt.rfa_records == [] and opt.rfa_trace == []      # today's weighted path


@pytest.mark.parametrize("T", [1, 2, 4])
def test_the_stage_follows_the_reference(T, cpu_engine):
    n = 7
    ups = _ups(n, numel=1023, seed=3)
    ups[4]["w"] = -3.0 * ups[4]["w"]                       # one far away
    base = {"w": torch.zeros(1023), "nbt": torch.tensor(100)}
    opt = _opt("fedavg", rfa=T)
    mc = type("MC", (), {"saved": [], "save": lambda self, *a: self.saved.append(a)})()
    opt.metric_collector = mc
    cache = _cache(ups, counts=[5 + 10 * i for i in range(n)])
    out = opt.do(base, cache, total=245)
    assert out is base and len(cache) == 0 and cache.pops == [f"e{i:02d}" for i in range(n)]
    assert cpu_engine["stats"] == [n] and len(cpu_engine["dist"]) == T - 1 and len(cpu_engine["reduce"]) == T - 1
    assert len(opt.rfa_trace) == T
    # each iteration's weights are the reference's of the reported distances, exactly; counts play no part
    prev = [1.0 / n] * n
    for d2, w in opt.rfa_trace:
        assert list(w) == R.weights(d2, 1e-6, prev)
        prev = list(w)
    assert list(opt.rfa_trace[0][0]) == R.dist2(ups, {"w": torch.zeros(1023)})[0]
    for (d2, w), (_, z) in zip(opt.rfa_trace[1:], cpu_engine["dist"]):
        assert list(d2) == R.dist2(ups, z)[0]
    for rates, (_, w) in zip(cpu_engine["reduce"], opt.rfa_trace):
        assert rates == list(w)
    rates, scales = cpu_engine["accumulate"][0]
    assert rates == list(opt.rfa_trace[-1][1]) and scales is None and abs(math.fsum(rates) - 1.0) < 1e-15
    assert rates[4] == min(rates)
    # near the fp64 reference iteration (the centre here is an fp32 tensor)
    w_ref, _ = R.geomedian([u["w"].double().numpy() for u in ups], T)
    assert np.allclose(rates, w_ref, rtol=1e-5)
    recs = opt.rfa_records
    assert [r.end for r in recs] == [f"e{i:02d}" for i in range(n)] and [r.weight for r in recs] == rates
    assert all(r.nonfinite == 0 and abs(r.norm - float(u["w"].double().norm())) < 1e-9 for r, u in zip(recs, ups))
    assert [r.dist for r in recs] == [math.sqrt(d) for d in opt.rfa_trace[-1][0]]
    assert ("rfa_iterations", "fedavg", T) in mc.saved and ("rfa_weight_min", "fedavg", min(rates)) in mc.saved
    assert ("rfa_dist_max", "fedavg", max(r.dist for r in recs)) in mc.saved
    assert opt.update_stats == []
    # the reference's empty rule is kept, and the records are this call's only
    assert opt.do(base, S.SortedCache(), total=5) is None and opt.rfa_records == [] and opt.rfa_trace == []
    assert opt.do(base, _cache(ups), total=0) is None and cpu_engine["stats"] == [n]


def test_all_beta_zero_stops_and_keeps_the_previous_weights(cpu_engine):
    n = 5
    ups = _ups(n, numel=16, seed=1)
    cpu_engine["dist_override"] = lambda ws, z: ([math.inf, math.nan, math.inf, math.inf, math.nan], [0] * n)
    opt = _opt("fedavg", rfa=6)
    opt.do({"w": torch.zeros(16), "nbt": torch.tensor(0)}, _cache(ups), total=n)
    assert len(cpu_engine["dist"]) == 1 and len(opt.rfa_trace) == 2         # stopped at t = 2
    (d1, w1), (d2, w2) = opt.rfa_trace
    assert w2 == w1 and not any(math.isfinite(d) for d in d2)
    assert cpu_engine["accumulate"][0][0] == list(w1)
    assert all(math.isnan(r.dist) or math.isinf(r.dist) for r in opt.rfa_records)
    # at t = 1 the previous weights are the equal weights
    from flame_amd.optimizer import rfa
    w, d, trace = rfa.iterate(ups, [math.inf] * n, 3, 1e-6)
    assert w == [0.2] * n and len(trace) == 1 and len(cpu_engine["dist"]) == 1


def test_an_empty_eligible_set_returns_none_with_the_base_untouched(cpu_engine):
    ups = _ups(6, numel=8)
    for u in ups:
        u["w"][3] = float("nan")
    for sort in ("fedavg", "fedadam"):
        for policy in ("keep", "skip"):
            opt = _opt(sort, rfa=3, nonfinite=policy)
            base = {"w": torch.ones(8), "nbt": torch.tensor(5)}
            cache = _cache(ups)
            assert opt.do(base, cache, total=6) is None and len(cache) == 0
            assert torch.equal(base["w"], torch.ones(8)) and int(base["nbt"]) == 5
            assert cpu_engine["accumulate"] == [] and cpu_engine["dist"] == [] and opt.rfa_trace == []
            assert [r.weight for r in opt.rfa_records] == [0.0] * 6 and all(r.nonfinite == 1 for r in opt.rfa_records)


def test_a_poisoned_update_is_left_out_under_every_policy(cpu_engine):
    n = 6
    ups = _ups(n, numel=32, seed=2)
    ups[2]["w"][5] = float("inf")
    for policy in ("keep", "skip"):
        opt = _opt("fedavg", rfa=2, nonfinite=policy)
        opt.do({"w": torch.zeros(32), "nbt": torch.tensor(0)}, _cache(ups), total=n)
        assert cpu_engine["dist"][-1][0] == n - 1 and len(cpu_engine["accumulate"][-1][0]) == n - 1
        assert opt.rfa_records[2].weight == 0.0 and opt.rfa_records[2].nonfinite == 1 and math.isnan(opt.rfa_records[2].dist)
        assert all(r.weight > 0 for i, r in enumerate(opt.rfa_records) if i != 2)
        assert (len(opt.update_stats) == n) == (policy == "skip")
    opt = _opt("fedavg", rfa=2, nonfinite="raise")
    with pytest.raises(ValueError, match="e02"):
        opt.do({"w": torch.zeros(32), "nbt": torch.tensor(0)}, _cache(ups), total=n)
    assert [r.nonfinite for r in opt.update_stats] == [int(i == 2) for i in range(n)] and opt.rfa_trace == []


def test_the_class_for_direct_use():
    import flame_amd.optimizers as fo
    from flame_amd.optimizer import FedAvg, FedGeoMedian
    g = FedGeoMedian()
    assert isinstance(g, FedAvg) and g.rfa == 5 and g.rfa_nu == 1e-6
    g = FedGeoMedian(iters=2, nu=1e-3, nonfinite="skip")
    assert g.rfa == 2 and g.rfa_nu == 1e-3 and g.guarded
    with pytest.raises(TypeError):
        FedGeoMedian(None)
    with pytest.raises(TypeError):
        FedGeoMedian(True)
    with pytest.raises(ValueError):
        FedGeoMedian(0)
    with pytest.raises(ValueError):
        FedGeoMedian(3, nu=0.0)
    assert FedGeoMedian not in fo.DROP_INS.values() and len(fo.DROP_INS) == 9


def test_kwargs_resolve_from_a_job_optimizer_block():
    import flame_amd.optimizers as fo
    provider = fo.install(fo.OptimizerProvider())
    for block, want in (('{"sort": "fedavg", "kwargs": {"rfa": 3}}', (3, 1e-6)),
                        ('{"sort": "fedadam", "kwargs": {"rfa": 5, "rfa_nu": 1e-4, "nonfinite": "skip"}}', (5, 1e-4)),
                        ('{"sort": "fedprox", "kwargs": {"mu": 0.01, "rfa": 1}}', (1, 1e-6))):
        job = json.loads(block)
        o = provider.get(job["sort"], **job["kwargs"])
        assert (o.rfa, o.rfa_nu) == want
        assert o.do({}, S.SortedCache(), total=0) is None


def test_engine_refuses_on_the_host():
    """engine.update_dist's own checks that need no device."""
    from flame_amd import engine
    d, nf = engine.update_dist([], {})
    assert d.shape == (0,) and nf.shape == (0,)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            engine.update_dist([{"w": torch.ones(8)} for _ in range(3)], {"w": torch.zeros(8)})
