"""The update guard's host side, without a GPU: the policy (``flame_amd/optimizer/guard.py``) and
the optimizers' control flow with ``engine.update_stats`` / ``engine.accumulate`` replaced by CPU
restatements; every refusal; the job-config path of the kwargs; the reference fixture."""
import json
import math

import numpy as np
import pytest
import torch

import scenarios as S


def _exact_stats(ws):
    """engine.update_stats on the CPU: fsum of the fp64 squares of the finite float elements."""
    sq, nf = [], []
    for w in ws:
        terms, bad = [], 0
        for k in w.keys():
            v = w[k]
            if not v.is_floating_point():
                continue
            x = v.double().reshape(-1)
            fin = torch.isfinite(x)
            bad += int((~fin).sum())
            terms.extend((x[fin] * x[fin]).tolist())
        sq.append(math.fsum(terms))
        nf.append(bad)
    return np.asarray(sq, np.float64), np.asarray(nf, np.int64)


@pytest.fixture
def cpu_engine(monkeypatch):
    """The engine's two device calls as CPU restatements (the oracle's arithmetic); records calls."""
    from flame_amd import engine
    from oracle import oracle as O
    calls = {"stats": 0, "accumulate": []}

    def update_stats(ws, device=None):
        calls["stats"] += 1
        return _exact_stats(list(ws))

    def accumulate(agg, entries, *, device=None, key_groups=None, after_group=None, scales=None):
        calls["accumulate"].append(([r for _, r in entries], None if scales is None else list(scales)))
        for i, (w, r) in enumerate(entries):
            for k, v in w.items():
                if scales is not None and v.is_floating_point():
                    v = O.tmp_tensor(v, scales[i])
                O.reduce_tensor(agg[k], [v], [r])

    monkeypatch.setattr(engine, "update_stats", update_stats)
    monkeypatch.setattr(engine, "accumulate", accumulate)
    return calls


def _opt(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _cache(ups, counts):
    c = S.SortedCache()
    for i, (u, n) in enumerate(zip(ups, counts)):
        c[f"e{i}"] = S.TR(u, n)
    return c


def test_scale_formula_and_boundary():
    from flame_amd.optimizer import guard
    assert guard.clip_scale(3.0, None) == 1.0
    assert guard.clip_scale(3.0, 3.0) == 1.0                      # `>`, not `>=` (differential_privacy.py:78)
    assert guard.clip_scale(math.nextafter(3.0, 4.0), 3.0) == 3.0 / (math.nextafter(3.0, 4.0) + 1e-6)
    assert guard.clip_scale(6.0, 3.0) == 3.0 / (6.0 + 1e-6)
    assert guard.clip_scale(0.0, 0.0) == 1.0 and guard.clip_scale(1e-30, 0.0) == 0.0
    recs, kept, total = guard.apply_policy(["a", "b", "c"], [1, 2, 3], [9.0, 36.0, 4.0], [0, 0, 0], 6, 3.0, "keep")
    assert kept == [0, 1, 2] and total == 6
    assert [r.scale for r in recs] == [1.0, 3.0 / (6.0 + 1e-6), 1.0]
    assert [r.norm for r in recs] == [3.0, 6.0, 2.0] and recs[1] == ("b", 2, 6.0, 0, 3.0 / (6.0 + 1e-6), False)


def test_policy_skip_raise_keep():
    from flame_amd.optimizer import guard
    args = (["a", "b", "c"], [1, 2, 3], [1.0, 4.0, 9.0], [0, 5, 0], 6)
    recs, kept, total = guard.apply_policy(*args, None, "skip")
    assert kept == [0, 2] and total == 4 and [r.skipped for r in recs] == [False, True, False]
    assert recs[1].nonfinite == 5 and recs[1].scale == 1.0
    recs, kept, total = guard.apply_policy(*args, 1.5, "keep")
    assert kept == [0, 1, 2] and total == 6 and not any(r.skipped for r in recs)
    assert [r.scale != 1.0 for r in recs] == [False, True, True]
    with pytest.raises(ValueError, match=r"\['b'\].*nothing was aggregated") as ei:
        guard.apply_policy(*args, None, "raise")
    assert isinstance(ei.value, guard.NonFiniteUpdate)
    assert [(r.end, r.nonfinite, r.skipped) for r in ei.value.records] == [("a", 0, False), ("b", 5, False), ("c", 0, False)]
    recs, kept, total = guard.apply_policy(["a"], [1], [1.0], [0], 1, None, "raise")      # nothing to raise about
    assert kept == [0] and total == 1


def test_fedavg_skip_renormalises_total(cpu_engine):
    g = torch.Generator().manual_seed(1)
    base = {"w": torch.randn(50, generator=g), "n": torch.tensor(3)}
    ups = [{"w": torch.randn(50, generator=g), "n": torch.tensor(i)} for i in range(4)]
    ups[2]["w"][7] = float("nan")
    counts = [10, 20, 30, 40]
    opt = _opt("fedavg", nonfinite="skip")
    cache = _cache(ups, counts)
    out = opt.do(base, cache, total=100)
    assert out is base and len(cache) == 0 and cpu_engine["stats"] == 1
    rates, scales = cpu_engine["accumulate"][0]
    assert rates == [10 / 70, 20 / 70, 40 / 70] and scales is None          # no clip: the plain reduction
    assert [r.skipped for r in opt.update_stats] == [False, False, True, False]
    assert bool(torch.isfinite(out["w"]).all())
    # every update skipped: None, as for an empty cache, and nothing accumulated
    opt = _opt("fedavg", nonfinite="skip")
    out = opt.do(base, _cache([ups[2]], [30]), total=30)
    assert out is None and len(cpu_engine["accumulate"]) == 1
    assert [r.skipped for r in opt.update_stats] == [True]


def test_fedavg_clip_passes_scales_and_raise_leaves_base(cpu_engine):
    g = torch.Generator().manual_seed(2)
    base = {"w": torch.randn(64, generator=g)}
    ups = [{"w": torch.randn(64, generator=g) * s} for s in (0.1, 1.0, 3.0)]
    opt = _opt("fedavg", clip_threshold=4.0)
    mc = type("MC", (), {"saved": [], "save": lambda self, *a: self.saved.append(a)})()
    opt.metric_collector = mc
    opt.do(base, _cache(ups, [1, 1, 2]), total=4)
    rates, scales = cpu_engine["accumulate"][0]
    norms = [math.sqrt(float(_exact_stats([u])[0][0])) for u in ups]
    assert rates == [0.25, 0.25, 0.5]
    assert scales == [1.0 if n <= 4.0 else 4.0 / (n + 1e-6) for n in norms] and scales[2] < 1.0 == scales[0]
    assert [tuple(r) for r in opt.update_stats] == [(f"e{i}", c, n, 0, s, False)
                                                    for i, (c, n, s) in enumerate(zip([1, 1, 2], norms, scales))]
    assert ("update_norm_max", "fedavg", max(norms)) in mc.saved
    assert ("updates_clipped", "fedavg", sum(s != 1.0 for s in scales)) in mc.saved
    assert ("updates_skipped", "fedavg", 0) in mc.saved
    # nobody above the threshold: scales stay away from the launch
    opt = _opt("fedavg", clip_threshold=1e9)
    opt.do(base, _cache(ups, [1, 1, 2]), total=4)
    assert cpu_engine["accumulate"][-1][1] is None
    # raise: before anything is written, entries popped
    ups[1]["w"][0] = float("inf")
    before = base["w"].clone()
    n_acc = len(cpu_engine["accumulate"])
    cache = _cache(ups, [1, 1, 2])
    with pytest.raises(ValueError, match="e1"):
        _opt("fedprox", mu=0.1, nonfinite="raise").do(base, cache, total=4)
    assert torch.equal(base["w"], before) and len(cache) == 0 and len(cpu_engine["accumulate"]) == n_acc
    # update_stats is the LAST do()'s: the raising call's records, then none for an empty round
    opt = _opt("fedavg", nonfinite="raise")
    opt.do(base, _cache(ups[:1], [1]), total=1)
    assert [r.end for r in opt.update_stats] == ["e0"]
    with pytest.raises(ValueError):
        opt.do(base, _cache(ups, [1, 1, 2]), total=4)
    assert [(r.end, r.nonfinite > 0) for r in opt.update_stats] == [("e0", False), ("e1", True), ("e2", False)]
    assert opt.do(base, S.SortedCache(), total=4) is None and opt.update_stats == []
    assert opt.do(base, _cache(ups[:1], [1]), total=0) is None and opt.update_stats == []


def test_eager_skip_corrects_only_its_own_call(cpu_engine):
    """The known limit: the eager role calls do() per arrival with ITS running total, so a skipped
    arrival's count is taken out of the call that skips it and of no later call."""
    g = torch.Generator().manual_seed(3)
    base = {"w": torch.zeros(8)}
    good = {"w": torch.randn(8, generator=g)}
    bad = {"w": torch.full((8,), float("nan"))}
    opt = _opt("fedavg", nonfinite="skip")
    assert opt.do(base, _cache([bad], [5]), total=5) is None                 # this call: corrected (nothing left)
    opt.do(base, _cache([good], [5]), total=10)                              # the role's total still counts the 5
    assert cpu_engine["accumulate"][-1][0] == [5 / 10]
    c = _cache([bad, good], [5, 15])
    opt.do(base, c, total=30)                                                # a call holding both: 15 / (30 - 5)
    assert cpu_engine["accumulate"][-1][0] == [15 / 25]


def test_defaults_run_no_new_code(monkeypatch):
    from flame_amd import engine
    monkeypatch.setattr(engine, "update_stats", lambda *a, **k: (_ for _ in ()).throw(AssertionError("called")))
    seen = []
    monkeypatch.setattr(engine, "accumulate", lambda agg, entries, **kw: seen.append(kw))
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5})):
        opt = _opt(sort, **kw)
        assert not opt.guarded and opt.clip_threshold is None and opt.nonfinite == "keep" and opt.update_stats == []
        opt.do({"w": torch.zeros(3)}, _cache([{"w": torch.ones(3)}], [1]), total=1)
        assert "scales" not in seen[-1]
    for sort in ("fedadam", "fedyogi", "fedadagrad"):
        assert not _opt(sort).guarded


def test_every_refusal():
    from flame_amd.optimizers import optimizer_provider as P
    from flame_amd.shard import ShardedOptimizer
    for sort, kw in (("fedavg", {"defer": True, "clip_threshold": 1.0}), ("fedavg", {"defer": True, "nonfinite": "skip"}),
                     ("fedadam", {"defer": True, "clip_threshold": 1.0}), ("fedyogi", {"defer": True, "nonfinite": "raise"}),
                     ("fedbuff", {"clip_threshold": 1.0}), ("fedbuff", {"nonfinite": "skip"}),
                     ("feddyn", {"alpha": 0.1, "clip_threshold": 1.0}), ("scaffold", {"k": 3, "nonfinite": "raise"})):
        with pytest.raises(NotImplementedError, match="update guard"):
            P.get(sort, **kw)
    with pytest.raises(NotImplementedError, match="all-reduce"):
        ShardedOptimizer(P.get("fedavg", clip_threshold=1.0))
    with pytest.raises(NotImplementedError, match="all-reduce"):
        ShardedOptimizer(P.get("fedadam", nonfinite="skip"))
    with pytest.raises(ValueError, match="nonfinite must be one of"):
        P.get("fedavg", nonfinite="drop")
    with pytest.raises(ValueError, match=">= 0"):
        P.get("fedavg", clip_threshold=-1.0)
    with pytest.raises(ValueError):
        P.get("fedadam", clip_threshold=float("nan"))
    with pytest.raises(TypeError):
        P.get("fedavg", clip_threshold="3")
    with pytest.raises(TypeError):
        P.get("fedavg", 0, 256, 1 << 30, 1.0)                  # keyword-only
    # the out-of-scope classes still construct with the defaults, and an unguarded optimizer still shards
    P.get("fedbuff"), P.get("feddyn", alpha=0.1), P.get("scaffold", k=3)
    assert P.get("fedbuff", clip_threshold=None, nonfinite="keep") is not None


def test_kwargs_resolve_from_a_job_optimizer_block():
    """A job's ``"optimizer": {"sort": ..., "kwargs": {...}}`` reaches the constructor through the
    provider ``install()`` fills, as ``defer`` does (syncfl/top_aggregator.py:97-99)."""
    import flame_amd.optimizers as fo
    provider = fo.install(fo.OptimizerProvider())
    job = json.loads('{"optimizer": {"sort": "fedavg", "kwargs": {"clip_threshold": 2.5, "nonfinite": "skip"}}}')
    o = provider.get(job["optimizer"]["sort"], **job["optimizer"]["kwargs"])
    assert type(o) is fo.DROP_INS["fedavg"] and o.guarded and o.clip_threshold == 2.5 and o.nonfinite == "skip"
    blocks = {"fedprox": {"mu": 0.01, "clip_threshold": 1}, "fedgft": {"fair": "SP", "gamma": 0.5, "nonfinite": "raise"},
              "fedadam": {"beta_1": 0.8, "clip_threshold": 10.0}, "fedyogi": {"clip_threshold": 0.5, "nonfinite": "skip"},
              "fedadagrad": {"nonfinite": "skip"}}
    for sort, kw in blocks.items():
        o = provider.get(sort, **json.loads(json.dumps(kw)))
        assert o.guarded and o.clip_threshold == (float(kw["clip_threshold"]) if "clip_threshold" in kw else None)
        assert o.nonfinite == kw.get("nonfinite", "keep")
        assert o.do({}, S.SortedCache(), total=0) is None           # usable with nothing received yet


def test_fedopt_guarded_round_takes_the_split_path(monkeypatch, cpu_engine):
    """A clipped FedOPT round: the scaled reduction, then the adaptive step with no clients; all
    updates skipped: current_weights unchanged and agg_weights None (fedopt.py:80-85)."""
    from flame_amd import engine
    from flame_amd.optimizer import fedopt as F
    seen = []
    monkeypatch.setattr(engine, "pick_device", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(engine, "reduce_", lambda outs, ins, clients, rates, **kw: seen.append(("reduce", len(clients[0]), kw)))
    monkeypatch.setattr(engine, "fedopt_reduce_adapt_",
                        lambda variant, avg_out, base, cur, cur_out, m, v, clients, rates, *a, **kw:
                        seen.append(("adapt", [len(c) for c in clients], list(rates))))
    monkeypatch.setattr(engine._Target, "__init__", lambda self, t, device: (setattr(self, "orig", t), setattr(self, "dev", t))[0])
    g = torch.Generator().manual_seed(4)
    opt = _opt("fedadam", clip_threshold=1.0, nonfinite="skip")
    base = {"w": torch.randn(16, generator=g)}
    opt._current = {"w": torch.randn(16, generator=g)}
    ups = [{"w": torch.randn(16, generator=g) * 5}, {"w": torch.randn(16, generator=g) * 0.01}]
    out = opt.do(base, _cache(ups, [1, 3]), total=4)
    assert [s[0] for s in seen] == ["reduce", "adapt"]
    assert seen[0][1] == 2 and seen[0][2]["scales"][0] < 1.0 == seen[0][2]["scales"][1]
    assert seen[1][1] == [0] and seen[1][2] == []
    assert list(out.keys()) == ["w"] and isinstance(opt, F.FedOPT)
    cur = opt.current_weights
    bad = [{"w": torch.full((16,), float("inf"))}]
    assert opt.do(base, _cache(bad, [2]), total=2) is cur and opt.agg_weights is None and len(seen) == 2


def test_reference_fixture_on_the_host(golden, cpu_engine):
    """fedavg_clipped.npz (the reference's own clip + FedAvg) through the drop-in's control flow
    with the CPU restatements: same clients clipped, scales within norm_tol, f32 key within
    2 * norm_tol + 2^-22."""
    import guard_fixture
    case = guard_fixture.load(golden("fedavg_clipped.npz"))
    assert len(case.updates) == 6 and sum(s != 1.0 for s in case.ref_scale) == 3
    assert {v.dtype for v in case.base.values()} == {torch.float32, torch.bfloat16}
    for u in case.updates:          # none within 1e-3 (relative) of the threshold
        n = math.sqrt(float(_exact_stats([u])[0][0]))
        assert abs(n - case.clip) / case.clip > 1e-3
    opt = _opt("fedavg", clip_threshold=case.clip)
    base = {k: v.clone() for k, v in case.base.items()}
    c = S.SortedCache()
    for i, (u, n) in enumerate(zip(case.updates, case.counts)):
        c[f"e{i}"] = S.TR(u, n)
    got = opt.do(base, c, total=sum(case.counts))
    guard_fixture.check(case, opt.update_stats, got)
