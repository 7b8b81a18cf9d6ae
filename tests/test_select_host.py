"""The ``trim_method`` kwarg's host side, without a GPU: validation, the routing between
``engine.trimmed_mean`` (the chain kernel) and ``engine.selected_mean`` (the radix-selection
kernel), the rounds refused with the cache still full, the records and metrics, that the default
runs none of the new code, ``engine.selected_mean``'s own refusals and its launch trace beside
``engine.trimmed_mean``'s.  Both engine functions are replaced by CPU restatements where a round
runs (tests/trimmed_ref.py, tests/select_ref.py)."""
import json

import numpy as np
import pytest
import torch

import scenarios as S
import select_ref as SR
import trimmed_ref as R


def _opt(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _cache(ups, counts=None):
    c = S.SortedCache()
    for i, u in enumerate(ups):
        c[f"e{i:03d}"] = S.TR(u, 1 if counts is None else counts[i])
    return c


def _ups(n, numel=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"w": torch.randn(numel, generator=g), "nbt": torch.tensor(3 + i)} for i in range(n)]


def _base(numel=12):
    return {"w": torch.zeros(numel), "nbt": torch.tensor(0)}


class _MC:
    def __init__(self):
        self.saved = []

    def save(self, mtype, alias, value):
        self.saved.append((mtype, alias, value))


@pytest.fixture
def cpu_means(monkeypatch):
    """engine.trimmed_mean / engine.selected_mean on the CPU; records (name, n, k) per call."""
    from flame_amd import engine
    calls = []

    def make(name, ref):
        def mean(agg, ws, k, *, init_first=False, device=None):
            ws = list(ws)
            calls.append((name, len(ws), k))
            for key, t in agg.items():
                if t.is_floating_point():
                    t.copy_(ref([w[key].reshape(-1) for w in ws], k, t.reshape(-1), t.dtype).view(t.shape))
                else:
                    for w in ws:
                        t += (w[key] * (1.0 / len(ws))).to(t.dtype)
        return mean

    monkeypatch.setattr(engine, "trimmed_mean", make("trimmed_mean", R.stream))
    monkeypatch.setattr(engine, "selected_mean", make("selected_mean", SR.select))
    return calls


def test_kwarg_validation():
    from flame_amd.optimizer import FedMedian, FedTrimmedMean, trim
    assert trim.check_method(None, None) is None and trim.check_method(None, 2) is None
    assert trim.check_method("select", 2) == "select" and trim.check_method("auto", "median") == "auto"
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5})):
        assert _opt(sort, trim=2, **kw).trim_method is None and _opt(sort, **kw).trim_method is None
        for m in ("select", "auto"):
            o = _opt(sort, trim=0.1, trim_method=m, **kw)
            assert o.trim_method == m and o.trim == 0.1 and o.trim_k is None and o.trim_kernel is None
        for bad in ("chain", "Select", "", "radix", "median"):
            with pytest.raises(ValueError, match="trim_method"):
                _opt(sort, trim=2, trim_method=bad, **kw)
        for bad in (1, True, 0.5, ["select"], b"select"):
            with pytest.raises(TypeError, match="trim_method"):
                _opt(sort, trim=2, trim_method=bad, **kw)
        for m in ("select", "auto"):
            with pytest.raises(ValueError, match="needs a trim"):
                _opt(sort, trim_method=m, **kw)
    with pytest.raises(ValueError):                                    # a bad trim is reported before the method
        _opt("fedavg", trim=0.5, trim_method="select")
    with pytest.raises(TypeError):                                     # keyword-only
        _opt("fedavg", False, 256, 1 << 30, None, "keep", 2, None, None, None, None, None, None, "select")
    assert FedMedian(trim_method="select").trim_method == "select" and FedMedian().trim_method is None
    assert FedTrimmedMean(0.2, trim_method="auto").trim_method == "auto"
    with pytest.raises(ValueError, match="trim_method"):
        FedMedian(trim_method="sort")
    with pytest.raises(TypeError):
        FedMedian("select")


def test_kwarg_resolves_from_a_job_optimizer_block():
    import flame_amd.optimizers as fo
    provider = fo.install(fo.OptimizerProvider())
    for block, want in (('{"sort": "fedavg", "kwargs": {"trim": "median", "trim_method": "select"}}', ("median", "select")),
                        ('{"sort": "fedprox", "kwargs": {"mu": 0.01, "trim": 0.1, "trim_method": "auto"}}', (0.1, "auto")),
                        ('{"sort": "fedavg", "kwargs": {"trim": 2, "trim_method": null}}', (2, None))):
        job = json.loads(block)
        o = provider.get(job["sort"], **job["kwargs"])
        assert (o.trim, o.trim_method) == want
        assert o.do({}, S.SortedCache(), total=0) is None


def test_every_existing_trim_refusal_still_applies():
    from flame_amd.optimizers import optimizer_provider as P
    from flame_amd.shard import ShardedOptimizer
    for m in ("select", "auto"):
        for sort, kw in (("fedavg", {"clip_threshold": 1.0}), ("fedprox", {"mu": 0.1, "clip_threshold": 2.0}),
                         ("fedgft", {"fair": "SP", "gamma": 0.5, "clip_threshold": 2.0}), ("fedavg", {"defer": True}),
                         ("fedavg", {"krum": 1}), ("fedavg", {"rfa": 3}), ("fedavg", {"noise_factor": 0.1})):
            with pytest.raises(NotImplementedError):
                P.get(sort, trim="median", trim_method=m, **kw)
        for sort in ("fedadam", "fedyogi", "fedadagrad"):
            with pytest.raises(TypeError, match="trim_method"):         # the FedOPT family refuses trim itself
                P.get(sort, trim=1, trim_method=m)
        with pytest.raises(NotImplementedError, match="trimmed-mean / median"):
            ShardedOptimizer(P.get("fedavg", trim=1, trim_method=m))
        opt = P.get("fedavg", trim="median", trim_method=m)
        cache = _cache(_ups(40))
        with pytest.raises(NotImplementedError, match="key groups"):
            opt.do(_base(), cache, total=40, flame_amd_key_groups=[["w"], ["nbt"]])
        assert len(cache) == 40


def test_default_runs_no_new_code(monkeypatch):
    """trim_method=None: neither new engine function is called, by a trimmed round or by a plain
    one, and the k > 16 refusal and its message are the chain kernel's."""
    from flame_amd import engine

    def boom(*a, **k):
        raise AssertionError("called")
    monkeypatch.setattr(engine, "selected_mean", boom)
    monkeypatch.setattr(engine, "select_max_clients", boom)
    seen = []
    monkeypatch.setattr(engine, "accumulate", lambda agg, entries, **kw: seen.append([r for _, r in entries]))
    trimmed = []
    monkeypatch.setattr(engine, "trimmed_mean", lambda agg, ws, k, **kw: trimmed.append((len(list(ws)), k)))
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5})):
        opt = _opt(sort, **kw)
        opt.do({"w": torch.zeros(3)}, _cache([{"w": torch.ones(3)}, {"w": torch.ones(3)}], [1, 3]), total=4)
        assert seen[-1] == [0.25, 0.75] and opt.trim_kernel is None
        opt = _opt(sort, trim="median", **kw)
        opt.metric_collector = mc = _MC()
        assert opt.do(_base(), _cache(_ups(34)), total=34) is not None
        assert trimmed[-1] == (34, 16) and opt.trim_k == 16 and opt.trim_kernel == "chain"
        assert [s[0] for s in mc.saved if s[0].startswith("trim")] == ["trim_k"]      # no new metric either
        cache = _cache(_ups(35))
        with pytest.raises(NotImplementedError, match=r"trim='median'.*k = 17.*capacity of 16.*n <= 34"):
            opt.do(_base(), cache, total=35)
        assert len(cache) == 35


def test_routing_records_and_metrics(cpu_means):
    for method, n, want in (("auto", 34, ("trimmed_mean", 34, 16, "chain")), ("auto", 35, ("selected_mean", 35, 17, "select")),
                            ("select", 34, ("selected_mean", 34, 16, "select")), ("select", 35, ("selected_mean", 35, 17, "select")),
                            ("select", 3, ("selected_mean", 3, 1, "select")), ("auto", 1, ("trimmed_mean", 1, 0, "chain"))):
        opt = _opt("fedavg", trim="median", trim_method=method)
        opt.metric_collector = mc = _MC()
        ups, base = _ups(n, seed=n), _base()
        ref = SR.select if want[0] == "selected_mean" else R.stream
        exp = ref([u["w"] for u in ups], want[2], base["w"].clone(), torch.float32)
        cache = _cache(ups)
        assert opt.do(base, cache, total=n) is base and len(cache) == 0
        assert cpu_means[-1] == want[:3] and opt.trim_k == want[2] and opt.trim_kernel == want[3]
        R.same_bits(f"{method} n={n}", base["w"], exp)
        for m in (("trim_k", "fedavg", want[2]), ("updates_trimmed_from", "fedavg", n), ("trim_kernel", "fedavg", want[3])):
            assert m in mc.saved, m
    # an int and a fraction beyond the chain's capacity; FedProx, FedGFT and the named classes route alike
    from flame_amd.optimizer import FedMedian, FedTrimmedMean
    for opt, n, want in ((_opt("fedprox", mu=0.1, trim=20, trim_method="auto"), 64, ("selected_mean", 64, 20)),
                         (_opt("fedgft", fair="SP", gamma=0.5, trim=0.45, trim_method="auto"), 100, ("selected_mean", 100, 45)),
                         (_opt("fedprox", mu=0.1, trim=0.1, trim_method="auto"), 100, ("trimmed_mean", 100, 10)),
                         (FedTrimmedMean(0.1, trim_method="select"), 100, ("selected_mean", 100, 10)),
                         (FedMedian(trim_method="auto"), 64, ("selected_mean", 64, 31))):
        assert opt.do(_base(4), _cache(_ups(n, numel=4)), total=n) is not None and cpu_means[-1] == want
    # the kernel of the LAST trimmed round
    opt = FedMedian(trim_method="auto")
    opt.do(_base(4), _cache(_ups(40, numel=4)), total=40)
    assert opt.trim_kernel == "select"
    opt.do(_base(4), _cache(_ups(9, numel=4)), total=9)
    assert opt.trim_kernel == "chain" and opt.trim_k == 4


@pytest.mark.parametrize("method", ["select", "auto"])
def test_round_refusals_leave_the_cache_full(method, monkeypatch, cpu_means):
    from flame_amd import engine
    for trim, n in ((4, 8), (4, 3), (1, 2), (1, 1), (20, 40)):
        opt = _opt("fedprox", mu=0.1, trim=trim, trim_method=method)
        cache, base = _cache(_ups(n, numel=3)), _base(3)
        with pytest.raises(ValueError, match=f"trim={trim}.*needs more than {2 * trim}"):
            opt.do(base, cache, total=n)
        assert len(cache) == n and list(cache.iterkeys()) == [f"e{i:03d}" for i in range(n)]
        assert float(base["w"].abs().sum()) == 0 and int(base["nbt"]) == 0 and opt.trim_k is None and opt.trim_kernel is None
    assert engine.select_max_clients() >= 4096
    monkeypatch.setattr(engine, "select_max_clients", lambda: 50)       # a small cap stands in for the kernel's
    opt = _opt("fedavg", trim="median", trim_method=method)
    cache = _cache(_ups(51, numel=3))
    with pytest.raises(NotImplementedError, match=r"trim_method=.*51 updates.*capacity of 50"):
        opt.do(_base(3), cache, total=51)
    assert len(cache) == 51 and cpu_means == []
    assert opt.do(_base(3), _cache(_ups(50, numel=3)), total=50) is not None and cpu_means == [("selected_mean", 50, 24)]
    if method == "auto":                                                # the chain has no cap on n
        assert _opt("fedavg", trim=2, trim_method="auto").do(_base(3), _cache(_ups(60, numel=3)), total=60) is not None
        assert cpu_means[-1] == ("trimmed_mean", 60, 2)


def test_nonfinite_skip_runs_first_and_k_follows_what_is_left(monkeypatch, cpu_means):
    from flame_amd import engine

    def stats(ws, device=None):
        ws = list(ws)
        return (np.asarray([float((w["w"][torch.isfinite(w["w"])].double() ** 2).sum()) for w in ws]),
                np.asarray([int((~torch.isfinite(w["w"])).sum()) for w in ws], np.int64))
    monkeypatch.setattr(engine, "update_stats", stats)
    ups = _ups(37)
    ups[3]["w"][:] = float("nan")
    ups[30]["w"][1] = float("inf")
    rest = [u for i, u in enumerate(ups) if i not in (3, 30)]
    base = _base()
    want = SR.select([u["w"] for u in rest], 17, base["w"].clone(), torch.float32)
    opt = _opt("fedavg", trim="median", trim_method="auto", nonfinite="skip")
    assert opt.do(base, _cache(ups), total=37) is base
    assert cpu_means == [("selected_mean", 35, 17)] and opt.trim_kernel == "select"       # 37 would have been k = 18
    assert [r.skipped for r in opt.update_stats] == [i in (3, 30) for i in range(37)]
    R.same_bits("skip", base["w"], want)
    ups = _ups(36)
    ups[0]["w"][0] = ups[1]["w"][0] = float("nan")
    opt.do(_base(), _cache(ups), total=36)                              # 34 left: the chain again
    assert cpu_means[-1] == ("trimmed_mean", 34, 16) and opt.trim_kernel == "chain"
    few = _ups(5)
    few[0]["w"][0] = few[1]["w"][0] = float("inf")
    with pytest.raises(ValueError, match="needs more than 4"):           # what is left is too few
        _opt("fedavg", trim=2, trim_method="select", nonfinite="skip").do(_base(), _cache(few), total=5)


def test_engine_refuses_on_the_host():
    """engine.selected_mean's own checks, all before any device is looked for."""
    from flame_amd import engine
    cap = engine.select_max_clients()
    assert cap >= 4096 and engine.trimmed_max_k() == 16
    agg = {"w": torch.zeros(8), "h": torch.zeros(4, dtype=torch.bfloat16), "nbt": torch.tensor(0)}
    ups = [{"w": torch.ones(8), "h": torch.ones(4, dtype=torch.bfloat16), "nbt": torch.tensor(1)} for _ in range(5)]
    for k in (3, -1):
        with pytest.raises(ValueError, match="selected_mean.*n > 2k"):
            engine.selected_mean(agg, ups, k)
    with pytest.raises(ValueError, match="n > 2k"):
        engine.selected_mean(agg, [], 0)
    with pytest.raises(NotImplementedError, match=f"capacity of {cap}"):
        engine.selected_mean(agg, ups[:1] * (cap + 1), 17)
    for bad in (1.0, True, "2", None):
        with pytest.raises(TypeError, match="selected_mean"):
            engine.selected_mean(agg, ups, bad)
    for bad in ({"w": torch.ones(8), "nbt": torch.tensor(1)},
                {"w": torch.ones(8), "h": torch.ones(4), "nbt": torch.tensor(1)},
                {"w": torch.ones(8), "h": torch.ones(4, dtype=torch.bfloat16), "x": torch.ones(2), "nbt": torch.tensor(1)}):
        with pytest.raises(ValueError, match="selected_mean.*float keys"):
            engine.selected_mean(agg, ups * 8 + [bad], 20)
    with pytest.raises(ValueError, match="init_first"):
        engine.selected_mean(agg, ups * 8, 19, init_first=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            engine.selected_mean(agg, ups * 8, 19)
        assert all(float(v.double().sum()) == 0 for v in agg.values())


def test_launch_trace_is_trimmed_means_but_for_the_name():
    """Under the launch-trace recorder, selected_mean uploads the same blocks and issues one launch
    per float dtype with trimmed_mean's arguments; the integer key goes last through reduce_ with
    rates 1 / n.  k = 2 is within both kernels' reach, k = 20 only within the selection's."""
    import test_engine_launch_trace as T
    from flame_amd import engine

    def selected(tr, n=5, k=2, **kw):
        agg = {nm: tr.t(f"agg.{nm}", torch.zeros(numel, dtype=dt)) for nm, dt, numel in T.TRIMMED_KEYS}
        with T._patched(engine, reduce_=tr.reduce_, select_max_clients=lambda: 65535):
            engine.selected_mean(agg, T._updates(tr, n, T.TRIMMED_KEYS), k, device=T.CPU, **kw)

    def run(fn, **opts):
        T.CASES["_select_probe"] = (fn, opts)
        try:
            return T.run_case("_select_probe")
        finally:
            del T.CASES["_select_probe"]

    for opts in ({}, {"xcd": 2}):
        sel = run(selected, **opts)
        ref = T.run_case("trimmed_mean_xcd" if opts else "trimmed_mean")
        assert "flame_agg_trimmed" not in json.dumps(sel)
        assert json.loads(json.dumps(sel).replace("flame_agg_select", "flame_agg_trimmed")) == ref
        assert [e[1] for e in T._calls(sel)] == ["flame_agg_select"] * 2 and sel[-1][0] == "reduce_"
        assert sel[-1][1:] == [["agg.nbt"], [[f"u{i}.nbt" for i in range(5)]], [(1.0 / 5).hex()] * 5, {}]
    big = run(lambda tr: selected(tr, n=45, k=20))
    calls = T._calls(big)
    assert [e[1] for e in calls] == ["flame_agg_select"] * 2
    assert [c[2][6:8] for c in calls] == [[45, 20], [45, 20]] and [c[2][-1] for c in calls] == [T.STREAM] * 2
    assert big[-1][0] == "reduce_" and big[-1][3] == [(1.0 / 45).hex()] * 45
