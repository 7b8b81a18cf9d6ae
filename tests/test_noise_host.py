"""``noise_factor`` / ``noise_seed`` on the host, without a GPU: the kwargs' validation, every refusal
(with the cache still full), the defaults running no new code, the job-config path, and the
``noise_round`` bookkeeping across empty, raising and normal rounds with the engine's device calls
replaced by CPU restatements (the oracle's arithmetic and tests/noise_ref.py)."""
import json
import math

import numpy as np
import pytest
import torch

import noise_ref as R
import scenarios as S


def _opt(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _cache(ups, counts):
    c = S.SortedCache()
    for i, (u, n) in enumerate(zip(ups, counts)):
        c[f"e{i}"] = S.TR(u, n)
    return c


@pytest.fixture
def cpu_engine(monkeypatch):
    """engine.accumulate and engine.noise_fill as CPU restatements; records the calls in order."""
    from flame_amd import engine
    from oracle import oracle as O
    calls = []

    def accumulate(agg, entries, *, device=None, key_groups=None, after_group=None, scales=None):
        calls.append(("accumulate", [r for _, r in entries], None if scales is None else list(scales)))
        for i, (w, r) in enumerate(entries):
            for k, v in w.items():
                if scales is not None and v.is_floating_point():
                    v = O.tmp_tensor(v, scales[i])
                O.reduce_tensor(agg[k], [v], [r])

    def noise_fill(like, seed, rnd, std, *, device=None):
        calls.append(("noise_fill", seed, rnd, std))
        return {k: R.fill_torch(t, seed, rnd, pos, 0, std) for pos, (k, t) in enumerate(like.items())
                if t.is_floating_point()}

    def update_stats(ws, device=None):      # engine.update_stats on the CPU (not recorded)
        sq, nf = [], []
        for w in ws:
            x = torch.cat([w[k].double().reshape(-1) for k in w.keys() if w[k].is_floating_point()])
            fin = torch.isfinite(x)
            sq.append(math.fsum((x[fin] * x[fin]).tolist()))
            nf.append(int((~fin).sum()))
        return np.asarray(sq, np.float64), np.asarray(nf, np.int64)

    monkeypatch.setattr(engine, "accumulate", accumulate)
    monkeypatch.setattr(engine, "noise_fill", noise_fill)
    monkeypatch.setattr(engine, "update_stats", update_stats)
    return calls


def test_kwarg_validation():
    from flame_amd.optimizer import noise
    assert noise.check_kwargs(None, None) == (None, None)
    assert noise.check_kwargs(0, None) == (None, None) and noise.check_kwargs(0.0, 7) == (None, 7)     # 0 is None
    assert noise.check_kwargs(2, 0) == (2.0, 0) and noise.check_kwargs(1e-3, (1 << 64) - 1) == (1e-3, (1 << 64) - 1)
    for bad in (True, False, "0.5", [0.5], 1j):
        with pytest.raises(TypeError, match="noise_factor"):
            noise.check_kwargs(bad, None)
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="noise_factor"):
            noise.check_kwargs(bad, None)
    for bad in (True, 1.0, "7"):
        with pytest.raises(TypeError, match="noise_seed"):
            noise.check_kwargs(0.5, bad)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="noise_seed"):
            noise.check_kwargs(0.5, bad)
    # None draws 8 bytes at construction and keeps them
    a, b = _opt("fedavg", noise_factor=0.5), _opt("fedavg", noise_factor=0.5)
    assert isinstance(a.noise_seed, int) and 0 <= a.noise_seed < 1 << 64 and a.noise_seed != b.noise_seed
    assert a.noise_factor == 0.5 and a.noise_round == 0 and a.noise_std is None
    o = _opt("fedavg")
    assert o.noise_factor is None and o.noise_seed is None and o.noise_round == 0
    assert _opt("fedavg", noise_factor=0).noise_factor is None
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5}), ("fedadam", {}),
                     ("fedyogi", {}), ("fedadagrad", {})):
        o = _opt(sort, noise_factor=0.25, noise_seed=11, **kw)
        assert (o.noise_factor, o.noise_seed, o.noise_round) == (0.25, 11, 0)
        with pytest.raises(TypeError):
            _opt(sort, noise_factor="1", **kw)
        with pytest.raises(ValueError):
            _opt(sort, noise_factor=-1, **kw)


def test_every_refusal_and_the_cache_stays_full():
    from flame_amd.optimizers import DROP_INS, optimizer_provider as P
    from flame_amd.optimizer import refusals
    from flame_amd.shard import ShardedOptimizer
    assert len(DROP_INS) == 9
    nf = {"noise_factor": 0.5}
    for sort, kw, why in (("fedavg", {"defer": True}, "not known when an arrival is queued"),
                          ("fedadam", {"defer": True}, "not known when an arrival is queued"),
                          ("fedyogi", {"defer": True}, "not known when an arrival is queued"),
                          ("fedavg", {"trim": 1}, "forms no entries"), ("fedprox", {"mu": 0.1, "trim": "median"}, "forms no entries"),
                          ("fedavg", {"krum": 1}, "no stated privacy meaning"), ("fedadam", {"krum": 1}, "no stated privacy meaning"),
                          ("fedavg", {"rfa": 3}, "no stated privacy meaning"), ("fedgft", {"fair": "SP", "gamma": 0.5, "rfa": 2},
                                                                                 "no stated privacy meaning")):
        with pytest.raises(NotImplementedError, match="noise_factor.*" + why):
            P.get(sort, **kw, **nf)
        P.get(sort, **kw)                                       # without the kwarg the same optimizer constructs
    for sort in ("fedavg", "fedadam"):
        with pytest.raises(NotImplementedError, match="noise_factor.*under sharding"):
            ShardedOptimizer(P.get(sort, **nf))
    for sort, kw in (("fedbuff", {}), ("feddyn", {"alpha": 0.1}), ("scaffold", {"k": 3})):
        with pytest.raises(TypeError):
            P.get(sort, noise_factor=0.5, **kw)
    assert {ctx for (f, ctx) in refusals.TABLE if f == "noise"} == {"defer", "trim", "krum", "rfa", "key_groups", "shard"}
    # the sharded wrapper's key groups reaching do(): refused before anything is popped
    opt = P.get("fedavg", **nf)
    cache = _cache([{"w": torch.ones(3)}, {"w": torch.ones(3)}], [1, 1])
    with pytest.raises(NotImplementedError, match="noise_factor"):
        opt.do({"w": torch.zeros(3)}, cache, total=2, flame_amd_key_groups=[["w"]])
    assert len(cache) == 2 and opt.noise_round == 0


def test_fedopt_key_groups_refused_with_the_cache_full(cpu_engine):
    opt = _opt("fedadam", noise_factor=0.5, noise_seed=1)
    base = {"w": torch.zeros(8)}
    opt.do(base, _cache([{"w": torch.ones(8)}], [1]), total=1)            # round 1: the passthrough, noised
    assert opt.noise_round == 1 and opt.current_weights is not None
    cache = _cache([{"w": torch.ones(8)}, {"w": torch.ones(8)}], [1, 1])
    with pytest.raises(NotImplementedError, match="noise_factor"):
        opt.do({"w": torch.zeros(8)}, cache, total=2, flame_amd_key_groups=[["w"]])
    assert len(cache) == 2 and opt.noise_round == 1


def test_defaults_run_no_new_code(monkeypatch):
    from flame_amd import engine

    def boom(*a, **k):
        raise AssertionError("engine.noise_fill called without noise_factor")

    monkeypatch.setattr(engine, "noise_fill", boom)
    monkeypatch.setattr(engine, "noise_fill_", boom)
    seen = []
    monkeypatch.setattr(engine, "accumulate", lambda agg, entries, **kw: seen.append(len(entries)))
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5}), ("fedadam", {}),
                     ("fedavg", {"noise_factor": 0}), ("fedavg", {"noise_factor": None, "noise_seed": 5})):
        opt = _opt(sort, **kw)
        opt.do({"w": torch.zeros(3)}, _cache([{"w": torch.ones(3)}], [1]), total=1)
        assert seen[-1] == 1 and opt.noise_round == 0 and opt.noise_std is None
    assert len(seen) == 6                                       # one reduction per round, nothing behind it


def test_kwargs_resolve_from_a_job_optimizer_block():
    import flame_amd.optimizers as fo
    provider = fo.install(fo.OptimizerProvider())
    job = json.loads('{"optimizer": {"sort": "fedavg", "kwargs": {"clip_threshold": 2.5, "noise_factor": 0.01, '
                     '"noise_seed": 12345678901234567890}}}')
    o = provider.get(job["optimizer"]["sort"], **job["optimizer"]["kwargs"])
    assert type(o) is fo.DROP_INS["fedavg"] and o.clip_threshold == 2.5
    assert o.noise_factor == 0.01 and o.noise_seed == 12345678901234567890
    blocks = {"fedprox": {"mu": 0.01, "noise_factor": 1}, "fedgft": {"fair": "SP", "gamma": 0.5, "noise_factor": 0.5},
              "fedadam": {"beta_1": 0.8, "noise_factor": 1e-3, "noise_seed": 3}, "fedyogi": {"noise_factor": 2.0},
              "fedadagrad": {"noise_factor": 0.125, "clip_threshold": 1.0}}
    for sort, kw in blocks.items():
        o = provider.get(sort, **json.loads(json.dumps(kw)))
        assert o.noise_factor == float(kw["noise_factor"]) and isinstance(o.noise_seed, int)
        assert o.do({}, S.SortedCache(), total=0) is None and o.noise_round == 0


def test_round_bookkeeping_and_the_noise_is_the_last_update(cpu_engine):
    """noise_round advances once per noised round -- not on an empty round, a total == 0 round or a
    round that raises; std = s * sqrt(fsum(rate^2)) over the kept rates; the noise is accumulated
    behind the entries with rate 1; the int key gets none."""
    from oracle import oracle as O
    g = torch.Generator().manual_seed(5)
    s, seed = 0.75, 1234 | 5678 << 32
    base = {"w": torch.randn(37, generator=g), "n": torch.tensor(3), "h": torch.randn(5, generator=g).to(torch.bfloat16)}
    ups = [{"w": torch.randn(37, generator=g), "n": torch.tensor(i), "h": torch.randn(5, generator=g).to(torch.bfloat16)}
           for i in range(4)]
    counts = [10, 20, 30, 40]
    opt = _opt("fedavg", noise_factor=s, noise_seed=seed, nonfinite="skip")
    mc = type("MC", (), {"saved": [], "save": lambda self, *a: self.saved.append(a)})()
    opt.metric_collector = mc
    assert opt.do(dict(base), S.SortedCache(), total=0) is None and opt.noise_round == 0            # empty
    assert opt.do(dict(base), _cache(ups, counts), total=0) is None and opt.noise_round == 0         # total == 0
    bad = {"w": torch.full((37,), float("nan")), "n": torch.tensor(0), "h": ups[0]["h"]}
    assert opt.do(dict(base), _cache([bad], [5]), total=5) is None and opt.noise_round == 0          # all skipped
    assert not cpu_engine

    got = {k: v.clone() for k, v in base.items()}
    ups[2]["w"][3] = float("inf")                                                                   # skipped
    out = opt.do(got, _cache(ups, counts), total=100)
    rates = [10 / 70, 20 / 70, 40 / 70]
    std = s * math.sqrt(math.fsum(r * r for r in rates))
    assert out is got and opt.noise_round == 1 and opt.noise_std == std
    assert [c[0] for c in cpu_engine] == ["accumulate", "noise_fill", "accumulate"]
    assert cpu_engine[0][1] == rates and cpu_engine[1] == ("noise_fill", seed, 0, std) and cpu_engine[2][1:] == ([1.0], None)
    assert ("noise_std", "fedavg", std) in mc.saved and ("noise_round", "fedavg", 0) in mc.saved
    want = {k: v.clone() for k, v in base.items()}
    kept = [ups[0], ups[1], ups[3]]
    for k in want:
        extra = [R.fill_torch(base[k], seed, 0, list(base).index(k), 0, std)] if base[k].is_floating_point() else []
        O.reduce_tensor(want[k], [u[k] for u in kept] + extra, rates + [1.0] * len(extra))
    S.assert_bitwise("noised round", got, want)

    # a round that raises does not advance the counter; the next normal round draws round 1
    with pytest.raises(KeyError):
        opt.do(got, _cache([{"w": ups[0]["w"], "zzz": torch.ones(1)}], [1]), total=1)
    assert opt.noise_round == 1
    del cpu_engine[:]
    opt.do(got, _cache(ups[:2], [1, 3]), total=4)
    assert opt.noise_round == 2 and cpu_engine[1] == ("noise_fill", seed, 1, s * math.sqrt(0.25 ** 2 + 0.75 ** 2))
