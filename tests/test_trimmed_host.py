"""The ``trim`` kwarg's host side, without a GPU: validation (``flame_amd/optimizer/trim.py``), the
trim count from an int / a fraction / ``"median"``, the rounds refused with the cache still full,
every refused combination, the metrics, and that the defaults run none of the new code.
``engine.trimmed_mean`` is replaced by the CPU restatement (tests/trimmed_ref.py)."""
import json

import pytest
import torch

import scenarios as S
import trimmed_ref as R


def _opt(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _cache(ups, counts=None):
    c = S.SortedCache()
    for i, u in enumerate(ups):
        c[f"e{i:02d}"] = S.TR(u, 1 if counts is None else counts[i])
    return c


def _ups(n, numel=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"w": torch.randn(numel, generator=g), "nbt": torch.tensor(3 + i)} for i in range(n)]


@pytest.fixture
def cpu_trimmed(monkeypatch):
    """engine.trimmed_mean on the CPU (float keys: the restatement; others: rate 1 / n); records calls."""
    from flame_amd import engine
    calls = []

    def trimmed_mean(agg, ws, k, *, init_first=False, device=None):
        ws = list(ws)
        calls.append((len(ws), k))
        for key, t in agg.items():
            if t.is_floating_point():
                t.copy_(R.stream([w[key].reshape(-1) for w in ws], k, t.reshape(-1), t.dtype).view(t.shape))
            else:
                for w in ws:
                    t += (w[key] * (1.0 / len(ws))).to(t.dtype)

    monkeypatch.setattr(engine, "trimmed_mean", trimmed_mean)
    return calls


def test_kwarg_validation():
    from flame_amd.optimizer import trim
    assert trim.check_kwarg(None) is None and trim.check_kwarg(0) == 0 and trim.check_kwarg(3) == 3
    assert trim.check_kwarg(0.0) == 0.0 and trim.check_kwarg(0.49) == 0.49 and trim.check_kwarg("median") == "median"
    for bad in (True, False):
        with pytest.raises(TypeError, match="bool"):
            _opt("fedavg", trim=bad)
    for bad in (-1, -0.1, 0.5, 0.75, 1.0, float("nan"), float("inf"), "mean", "Median", ""):
        with pytest.raises(ValueError):
            _opt("fedavg", trim=bad)
    for bad in ([1], (2,), {"k": 1}, 1 + 0j, b"median"):
        with pytest.raises(TypeError):
            _opt("fedavg", trim=bad)
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5})):
        o = _opt(sort, trim=2, **kw)
        assert o.trim == 2 and o.trim_k is None
        assert _opt(sort, **kw).trim is None
    with pytest.raises(TypeError):
        _opt("fedavg", False, 256, 1 << 30, None, "keep", 2)          # keyword-only, like the guard's kwargs


def test_trim_count_from_int_fraction_and_median():
    from flame_amd.optimizer import trim
    want_median = {1: 0, 2: 0, 3: 1, 4: 1, 9: 4, 10: 4, 34: 16}
    for n, k in want_median.items():
        assert trim.count("median", n) == k
        assert n - 2 * k == (1 if n % 2 else 2)                       # one value kept for odd n, two for even
        assert trim.check_round("median", n, 16) == k
    for n in want_median:
        assert trim.count(0, n) == 0 and trim.count(3, n) == 3        # an int is k itself
        assert trim.count(0.0, n) == 0
        assert trim.count(0.25, n) == n // 4                          # floor(trim * n), exact for a dyadic fraction
        assert trim.count(0.1, n) == {1: 0, 2: 0, 3: 0, 4: 0, 9: 0, 10: 1, 34: 3}[n]
        assert trim.count(0.49, n) == {1: 0, 2: 0, 3: 1, 4: 1, 9: 4, 10: 4, 34: 16}[n]
    with pytest.raises(NotImplementedError, match="capacity of 16"):
        trim.check_round("median", 35, 16)                            # k = 17
    with pytest.raises(ValueError, match="needs more than 6"):
        trim.check_round(3, 6, 16)
    assert trim.check_round(3, 7, 16) == 3


def test_classes_for_direct_use():
    import flame_amd.optimizers as fo
    from flame_amd.optimizer import FedAvg, FedMedian, FedTrimmedMean
    t, m = FedTrimmedMean(0.2), FedMedian()
    assert isinstance(t, FedAvg) and t.trim == 0.2 and isinstance(m, FedTrimmedMean) and m.trim == "median"
    assert FedTrimmedMean(1, nonfinite="skip").nonfinite == "skip" and FedMedian(nonfinite="raise").guarded
    with pytest.raises(TypeError):
        FedTrimmedMean(None)
    with pytest.raises(TypeError):
        FedTrimmedMean()
    with pytest.raises(ValueError):
        FedTrimmedMean(0.5)
    assert FedTrimmedMean not in fo.DROP_INS.values() and FedMedian not in fo.DROP_INS.values()
    assert len(fo.DROP_INS) == 9


@pytest.mark.parametrize("trim,n,exc", [(4, 8, ValueError), (4, 3, ValueError), (1, 2, ValueError), (1, 1, ValueError),
                                        (17, 40, NotImplementedError), (0.45, 40, NotImplementedError),
                                        ("median", 35, NotImplementedError)])
def test_unusable_rounds_raise_with_the_cache_still_full(trim, n, exc, cpu_trimmed):
    """n <= 2k (an int k only: floor(trim * n) of a fraction below 0.5 and the median always leave
    something) and k > 16 are raised before anything is popped."""
    opt = _opt("fedprox", mu=0.1, trim=trim)
    cache = _cache(_ups(n, numel=6))
    base = {"w": torch.zeros(6), "nbt": torch.tensor(0)}
    with pytest.raises(exc, match="trim="):
        opt.do(base, cache, total=n)
    assert len(cache) == n and list(cache.iterkeys()) == [f"e{i:02d}" for i in range(n)]     # nothing popped
    assert float(base["w"].abs().sum()) == 0 and int(base["nbt"]) == 0 and cpu_trimmed == [] and opt.trim_k is None


def test_median_beyond_34_updates_is_refused_by_name(cpu_trimmed):
    from flame_amd.optimizer import FedMedian
    opt = FedMedian()
    cache = _cache(_ups(35, numel=4))
    with pytest.raises(NotImplementedError, match=r"trim='median'.*k = 17.*capacity of 16"):
        opt.do({"w": torch.zeros(4), "nbt": torch.tensor(0)}, cache, total=35)
    assert len(cache) == 35
    base = {"w": torch.zeros(4), "nbt": torch.tensor(0)}
    assert opt.do(base, _cache(_ups(34, numel=4)), total=34) is base and cpu_trimmed == [(34, 16)]


def test_do_pops_in_order_trims_in_place_and_records_metrics(cpu_trimmed):
    ups = _ups(9)
    base = {"w": torch.randn(40, generator=torch.Generator().manual_seed(5)), "nbt": torch.tensor(100)}
    want = R.stream([u["w"] for u in ups], 2, base["w"], torch.float32)
    opt = _opt("fedavg", trim=2)
    mc = type("MC", (), {"saved": [], "save": lambda self, *a: self.saved.append(a)})()
    opt.metric_collector = mc
    cache = _cache(ups, counts=[5 + i for i in range(9)])
    popped = []
    pop = cache.pop
    cache.pop = lambda k, d=None: (popped.append(k), pop(k, d))[1]
    out = opt.do(base, cache, total=81)
    assert out is base and opt.agg_weights is base and len(cache) == 0
    assert popped == [f"e{i:02d}" for i in range(9)] and cpu_trimmed == [(9, 2)] and opt.trim_k == 2
    R.same_bits("w", base["w"], want)
    assert ("trim_k", "fedavg", 2) in mc.saved and ("updates_trimmed_from", "fedavg", 9) in mc.saved
    # the reference's empty rule is kept
    assert opt.do(base, S.SortedCache(), total=5) is None and opt.do(base, _cache(ups), total=0) is None
    assert cpu_trimmed == [(9, 2)]
    # a fraction and the median resolve per round
    assert _opt("fedavg", trim=0.25).do(base, _cache(ups), total=9) is base and cpu_trimmed[-1] == (9, 2)
    assert _opt("fedavg", trim="median").do(base, _cache(_ups(10)), total=10) is base and cpu_trimmed[-1] == (10, 4)


def test_nonfinite_policies_run_first(monkeypatch, cpu_trimmed):
    import numpy as np
    from flame_amd import engine

    def stats(ws, device=None):
        ws = list(ws)
        return (np.asarray([float((w["w"][torch.isfinite(w["w"])].double() ** 2).sum()) for w in ws]),
                np.asarray([int((~torch.isfinite(w["w"])).sum()) for w in ws], np.int64))
    monkeypatch.setattr(engine, "update_stats", stats)
    ups = _ups(9)
    ups[3]["w"][:] = float("nan")
    base = {"w": torch.zeros(40), "nbt": torch.tensor(0)}
    want = R.stream([u["w"] for i, u in enumerate(ups) if i != 3], 2, base["w"].clone(), torch.float32)
    opt = _opt("fedavg", trim=0.25, nonfinite="skip")
    assert opt.do(base, _cache(ups), total=9) is base
    assert cpu_trimmed == [(8, 2)] and [r.skipped for r in opt.update_stats] == [i == 3 for i in range(9)]
    R.same_bits("skip", base["w"], want)
    # what remains can be too few: the round raises after the guard popped, as the guard's own "raise" does
    few = _ups(5)
    few[0]["w"][0] = few[1]["w"][0] = float("inf")
    cache = _cache(few)
    with pytest.raises(ValueError, match="needs more than 2"):
        _opt("fedavg", trim=1, nonfinite="skip").do(base, _cache(few[:3]), total=3)
    with pytest.raises(ValueError, match="non-finite"):
        _opt("fedavg", trim=1, nonfinite="raise").do(base, cache, total=5)
    assert len(cpu_trimmed) == 1
    # every update skipped: None
    assert _opt("fedavg", trim=0, nonfinite="skip").do(base, _cache(few[:2]), total=2) is None


def test_every_refusal():
    from flame_amd.optimizers import optimizer_provider as P
    from flame_amd.shard import ShardedOptimizer
    for sort, kw in (("fedavg", {"clip_threshold": 1.0}), ("fedprox", {"mu": 0.1, "clip_threshold": 2.0}),
                     ("fedgft", {"fair": "SP", "gamma": 0.5, "clip_threshold": 2.0}), ("fedavg", {"defer": True}),
                     ("fedadam", {}), ("fedyogi", {}), ("fedadagrad", {}), ("fedadam", {"defer": True})):
        for trim in (1, 0.1, "median", 0):
            with pytest.raises(NotImplementedError, match="trimmed-mean / median"):
                P.get(sort, trim=trim, **kw)
    for sort, kw in (("fedbuff", {}), ("feddyn", {"alpha": 0.1}), ("scaffold", {"k": 3})):
        with pytest.raises(TypeError, match="trim"):
            P.get(sort, trim=1, **kw)                                   # these do not take the kwarg
    with pytest.raises(NotImplementedError, match="trimmed-mean / median"):
        ShardedOptimizer(P.get("fedavg", trim=1))
    opt = P.get("fedavg", trim=1)
    cache = _cache(_ups(5))
    with pytest.raises(NotImplementedError, match="key groups"):
        opt.do({"w": torch.zeros(40), "nbt": torch.tensor(0)}, cache, total=5, flame_amd_key_groups=[["w"], ["nbt"]])
    assert len(cache) == 5
    with pytest.raises(ValueError):                                     # a bad value is a bad value before it is refused
        P.get("fedadam", trim=0.5)
    # trim=None changes nothing anywhere
    assert P.get("fedadam", trim=None).trim is None and P.get("fedavg", clip_threshold=1.0, trim=None).guarded


def test_defaults_run_no_new_code(monkeypatch):
    from flame_amd import engine
    monkeypatch.setattr(engine, "trimmed_mean", lambda *a, **k: (_ for _ in ()).throw(AssertionError("called")))
    monkeypatch.setattr(engine, "trimmed_max_k", lambda: (_ for _ in ()).throw(AssertionError("called")))
    seen = []
    monkeypatch.setattr(engine, "accumulate", lambda agg, entries, **kw: seen.append([r for _, r in entries]))
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5})):
        opt = _opt(sort, **kw)
        assert opt.trim is None and opt.trim_k is None
        opt.do({"w": torch.zeros(3)}, _cache([{"w": torch.ones(3)}, {"w": torch.ones(3)}], [1, 3]), total=4)
        assert seen[-1] == [0.25, 0.75]                                 # today's weighted path


def test_kwarg_resolves_from_a_job_optimizer_block():
    import flame_amd.optimizers as fo
    provider = fo.install(fo.OptimizerProvider())
    for block, want in (('{"sort": "fedavg", "kwargs": {"trim": 2}}', 2),
                        ('{"sort": "fedavg", "kwargs": {"trim": 0.1, "nonfinite": "skip"}}', 0.1),
                        ('{"sort": "fedprox", "kwargs": {"mu": 0.01, "trim": "median"}}', "median")):
        job = json.loads(block)
        o = provider.get(job["sort"], **job["kwargs"])
        assert o.trim == want and type(o.trim) is type(want)
        assert o.do({}, S.SortedCache(), total=0) is None


def test_engine_refuses_on_the_host():
    """engine.trimmed_mean's own checks, all before any device is looked for."""
    from flame_amd import engine
    agg = {"w": torch.zeros(8), "h": torch.zeros(4, dtype=torch.bfloat16), "nbt": torch.tensor(0)}
    ups = [{"w": torch.ones(8), "h": torch.ones(4, dtype=torch.bfloat16), "nbt": torch.tensor(1)} for _ in range(5)]
    with pytest.raises(ValueError, match="n > 2k"):
        engine.trimmed_mean(agg, ups, 3)
    with pytest.raises(ValueError, match="n > 2k"):
        engine.trimmed_mean(agg, ups, -1)
    with pytest.raises(ValueError, match="n > 2k"):
        engine.trimmed_mean(agg, [], 0)
    with pytest.raises(NotImplementedError, match="capacity 16"):
        engine.trimmed_mean(agg, ups * 10, 17)
    with pytest.raises(TypeError):
        engine.trimmed_mean(agg, ups, 1.0)
    with pytest.raises(TypeError):
        engine.trimmed_mean(agg, ups, True)
    for bad in ({"w": torch.ones(8), "nbt": torch.tensor(1)},                                        # a float key missing
                {"w": torch.ones(8), "h": torch.ones(4), "nbt": torch.tensor(1)},                    # another dtype
                {"w": torch.ones(8), "h": torch.ones(4, dtype=torch.bfloat16), "x": torch.ones(2), "nbt": torch.tensor(1)}):
        with pytest.raises(ValueError, match="float keys"):
            engine.trimmed_mean(agg, ups[:4] + [bad], 1)
    with pytest.raises(ValueError, match="init_first"):
        engine.trimmed_mean(agg, ups, 1, init_first=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            engine.trimmed_mean(agg, ups, 1)
        assert all(float(v.double().sum()) == 0 for v in agg.values())
