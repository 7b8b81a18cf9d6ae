"""The ``krum`` / ``krum_select`` kwargs' host side, without a GPU: validation
(``flame_amd/optimizer/krum.py``), the f / q / m arithmetic, the rounds refused with the cache still
full, ties, ineligible updates, every refused combination, the metrics and records, ``select`` on
hand-made Gram matrices against tests/krum_ref.py, and that the defaults run none of the new code.
``engine.update_gram`` is replaced by a CPU Gram matrix and ``engine.accumulate`` by a recorder."""
import json
import math

import numpy as np
import pytest
import torch

import krum_ref as R
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


def _ups(n, numel=40, seed=0, f=0):
    g = torch.Generator().manual_seed(seed)
    ups, _ = R.honest_bad(g, n, f, (numel,))
    return [{"w": u["k0"].float(), "nbt": torch.tensor(3 + i)} for i, u in enumerate(ups)]


@pytest.fixture
def cpu_engine(monkeypatch):
    """engine.update_gram on the CPU (X X^T of the sanitised float elements), engine.accumulate as
    the reference's statement in torch-CPU ops, engine.gram_max_clients = 1024; records the calls."""
    from flame_amd import engine
    calls = {"gram": [], "accumulate": [], "stats": 0}

    def update_gram(ws, device=None):
        ws = list(ws)
        calls["gram"].append(len(ws))
        flat = [R.flatten(w) for w in ws]
        x = np.stack([v for v, _ in flat])
        return x @ x.T, np.asarray([b for _, b in flat], np.int64)

    def accumulate(agg, entries, **kw):
        calls["accumulate"].append(([r for _, r in entries], kw.get("scales")))
        for i, (w, r) in enumerate(entries):
            sc = 1.0 if kw.get("scales") is None else kw["scales"][i]
            for k, t in agg.items():
                v = w[k] * sc if w[k].is_floating_point() else w[k]
                t += (v * r).to(w[k].dtype)

    def update_stats(ws, device=None):
        calls["stats"] += 1
        raise AssertionError("a krum round launches no flame_update_stats")

    monkeypatch.setattr(engine, "update_gram", update_gram)
    monkeypatch.setattr(engine, "accumulate", accumulate)
    monkeypatch.setattr(engine, "update_stats", update_stats)
    monkeypatch.setattr(engine, "gram_max_clients", lambda: 1024)
    return calls


def test_kwarg_validation():
    from flame_amd.optimizer import krum
    assert krum.check_kwargs(None, None) == (None, None)
    assert krum.check_kwargs(0, None) == (0, None) and krum.check_kwargs(3, 2) == (3, 2)
    assert krum.check_kwargs(0.0, None) == (0.0, None) and krum.check_kwargs(0.49, 1) == (0.49, 1)
    for bad in (True, False):
        with pytest.raises(TypeError, match="bool"):
            _opt("fedavg", krum=bad)
        with pytest.raises(TypeError):
            _opt("fedavg", krum=1, krum_select=bad)
    for bad in (-1, -0.1, 0.5, 0.75, 1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _opt("fedavg", krum=bad)
    for bad in ("2", [1], (2,), {"f": 1}, 1 + 0j):
        with pytest.raises(TypeError):
            _opt("fedavg", krum=bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="krum_select"):
            _opt("fedavg", krum=1, krum_select=bad)
    for bad in (1.0, "1", [1]):
        with pytest.raises(TypeError, match="krum_select"):
            _opt("fedavg", krum=1, krum_select=bad)
    with pytest.raises(ValueError, match="needs krum"):
        _opt("fedavg", krum_select=1)
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5}),
                     ("fedadam", {}), ("fedyogi", {}), ("fedadagrad", {})):
        o = _opt(sort, krum=2, krum_select=3, **kw)
        assert o.krum == 2 and o.krum_select == 3 and o.krum_records == []
        assert _opt(sort, **kw).krum is None
    with pytest.raises(TypeError):
        _opt("fedavg", False, 256, 1 << 30, None, "keep", None, 2)       # keyword-only, like the guard's kwargs


def test_f_q_m_arithmetic():
    from flame_amd.optimizer import krum
    assert krum.check_round(0, None, 3, 1024) == (0, 1, 3)
    assert krum.check_round(1, None, 5, 1024) == (1, 2, 4)
    assert krum.check_round(2, None, 9, 1024) == (2, 5, 7)
    assert krum.check_round(2, 1, 9, 1024) == (2, 5, 1)
    assert krum.check_round(2, 7, 9, 1024) == (2, 5, 7)
    assert krum.check_round(31, None, 130, 1024) == (31, 97, 99)
    assert krum.check_round(0.25, None, 9, 1024) == (2, 5, 7)           # floor(0.25 * 9) = 2
    assert krum.check_round(0.2, None, 10, 1024) == (2, 6, 8)
    assert krum.check_round(0.49, None, 101, 1024) == (49, 50, 52)
    assert krum.check_round(510, None, 1024, 1024) == (510, 512, 514)
    with pytest.raises(ValueError, match=r"2f \+ 3 = 7"):
        krum.check_round(2, None, 6, 1024)
    with pytest.raises(ValueError, match=r"2f \+ 3"):
        krum.check_round(0, None, 2, 1024)
    with pytest.raises(ValueError, match=r"2f \+ 3"):
        krum.check_round(0.49, None, 9, 1024)                           # f = 4 needs 11
    with pytest.raises(ValueError, match="krum_select"):
        krum.check_round(2, 8, 9, 1024)                                 # m > n - f
    with pytest.raises(NotImplementedError, match="capacity of 1024"):
        krum.check_round(1, None, 1025, 1024)
    with pytest.raises(NotImplementedError, match="capacity of 64"):
        krum.check_round(1, None, 65, 64)


@pytest.mark.parametrize("krum,select,n,exc", [(2, None, 6, ValueError), (1, None, 4, ValueError), (0, None, 2, ValueError),
                                               (0.45, None, 9, ValueError), (2, 8, 9, ValueError),
                                               (1, None, 1025, NotImplementedError)])
def test_unusable_rounds_raise_before_a_pop(krum, select, n, exc, cpu_engine):
    for sort, kw in (("fedavg", {}), ("fedadam", {})):
        opt = _opt(sort, krum=krum, krum_select=select, **kw)
        cache = _cache(_ups(n, numel=4))
        base = {"w": torch.zeros(4), "nbt": torch.tensor(0)}
        with pytest.raises(exc, match="krum"):
            opt.do(base, cache, total=n)
        assert cache.pops == [] and len(cache) == n
        assert float(base["w"].abs().sum()) == 0 and int(base["nbt"]) == 0
        assert cpu_engine["gram"] == [] and cpu_engine["accumulate"] == [] and opt.krum_records == []


def test_do_selects_the_honest_updates_and_records(cpu_engine):
    n, f = 9, 2
    ups = _ups(n, numel=1023, seed=4, f=f)
    honest = [i for i in range(n) if i not in R.bad_positions(n, f)]
    base = {"w": torch.zeros(1023), "nbt": torch.tensor(100)}
    opt = _opt("fedavg", krum=f)
    mc = type("MC", (), {"saved": [], "save": lambda self, *a: self.saved.append(a)})()
    opt.metric_collector = mc
    cache = _cache(ups, counts=[5 + i for i in range(n)])
    out = opt.do(base, cache, total=81)
    assert out is base and opt.agg_weights is base and len(cache) == 0
    assert cache.pops == [f"e{i:02d}" for i in range(n)] and cpu_engine["gram"] == [n] and cpu_engine["stats"] == 0
    rates, scales = cpu_engine["accumulate"][0]
    assert rates == [1.0 / 7] * 7 and scales is None                    # counts and total play no part
    recs = opt.krum_records
    assert [r.end for r in recs] == [f"e{i:02d}" for i in range(n)]
    assert [i for i, r in enumerate(recs) if r.selected] == honest
    ref_scores, ref_sel, _, _ = R.krum(ups, f)
    assert ref_sel == honest
    assert all(abs(r.score - s) <= 1e-10 * s for r, s in zip(recs, ref_scores))
    assert all(r.nonfinite == 0 and abs(r.norm - math.sqrt(float((u["w"].double() ** 2).sum()))) < 1e-9
               for r, u in zip(recs, ups))
    finite = [r.score for r in recs]
    assert ("krum_selected", "fedavg", 7) in mc.saved and ("krum_f", "fedavg", 2) in mc.saved
    assert ("krum_score_max", "fedavg", max(finite)) in mc.saved
    assert opt.update_stats == []
    # the reference's empty rule is kept, and the records are this call's only
    assert opt.do(base, S.SortedCache(), total=5) is None and opt.krum_records == []
    assert opt.do(base, _cache(ups), total=0) is None and cpu_engine["gram"] == [n]
    # krum_select=1: the single lowest score
    one = _opt("fedavg", krum=f, krum_select=1)
    one.do({"w": torch.zeros(1023), "nbt": torch.tensor(0)}, _cache(ups), total=n)
    assert [i for i, r in enumerate(one.krum_records) if r.selected] == [int(np.argmin(ref_scores))]
    assert cpu_engine["accumulate"][-1][0] == [1.0]
    # a fraction resolves per round
    frac = _opt("fedprox", mu=0.1, krum=0.25)
    frac.do({"w": torch.zeros(1023), "nbt": torch.tensor(0)}, _cache(ups), total=n)
    assert [i for i, r in enumerate(frac.krum_records) if r.selected] == honest


def test_select_on_hand_made_gram_matrices():
    from flame_amd.optimizer import krum
    # five points on a line: 0, 1, 2, 3 and 10 (the outlier); G = x x^T
    x = np.array([0.0, 1.0, 2.0, 3.0, 10.0])
    gram = np.outer(x, x)
    nf = np.zeros(5, np.int64)
    d, ok = krum.distances(gram, nf, None)
    assert ok.all() and d[0, 4] == 100.0 and d[1, 3] == 4.0 and d[2, 2] == 0.0
    sc, sel = krum.select(gram, nf, None, 1, 4)                          # q = 2
    assert sc == [1.0 + 4.0, 1.0 + 1.0, 1.0 + 1.0, 1.0 + 4.0, 49.0 + 64.0] and sel == [0, 1, 2, 3]
    ups = [{"w": torch.tensor([v])} for v in x]
    sc_ref, sel_ref, d_ref, _ = R.krum(ups, 1)
    assert sc == sc_ref and sel == sel_ref and np.array_equal(d, d_ref)
    # ties go to the earlier cache position (a stable sort): 1 and 2 tie for the lowest score
    assert krum.select(gram, nf, None, 1, 1)[1] == [1] and R.select(d_ref, 1, 1)[1] == [1]
    assert krum.select(gram, nf, None, 1, 3)[1] == [0, 1, 2]            # then 0 before 3
    # four equal updates and one far away: all scores of the four are 0, the first m are taken
    same = np.outer([1.0, 1.0, 1.0, 1.0, 5.0], [1.0, 1.0, 1.0, 1.0, 5.0])
    assert krum.select(same, nf, None, 1, 2) == ([0.0, 0.0, 0.0, 0.0, 32.0], [0, 1])
    # the clip scales make the distances those of the scaled updates
    s = [1.0, 1.0, 1.0, 1.0, 0.25]
    d, _ = krum.distances(gram, nf, s)
    assert d[0, 4] == 6.25 and d[3, 4] == 0.25 and d[0, 3] == 9.0
    assert np.array_equal(d, R.distances([{"w": torch.tensor([v], dtype=torch.float64)} for v in x], s)[0])
    # a negative rounding residue is clamped to 0
    near = np.array([[1.0, 1.0 + 2 ** -52], [1.0 + 2 ** -52, 1.0]])
    assert krum.distances(near, np.zeros(2, np.int64), None)[0][0, 1] == 0.0


def test_ineligible_updates_are_never_selected():
    from flame_amd.optimizer import krum
    x = np.array([0.0, 1.0, 2.0, 3.0, 1.5, 2.5, 0.5])
    gram = np.outer(x, x)
    nf = np.array([0, 0, 3, 0, 0, 0, 0], np.int64)                      # update 2 holds non-finite elements
    d, ok = krum.distances(gram, nf, None)
    assert ok.tolist() == [True, True, False, True, True, True, True]
    assert np.isinf(d[2]).all() and np.isinf(d[:, 2]).all()
    sc, sel = krum.select(gram, nf, None, 2, 5)                          # q = 3
    assert math.isinf(sc[2]) and 2 not in sel and len(sel) == 5 and all(math.isfinite(sc[i]) for i in sel)
    # a non-finite diagonal (an f64 key that overflowed) is ineligible as well
    g2 = gram.copy()
    g2[5, 5] = math.inf
    g2[5, :5] = g2[:5, 5] = math.nan
    sc, sel = krum.select(g2, np.zeros(7, np.int64), None, 2, 5)
    assert math.isinf(sc[5]) and 5 not in sel and len(sel) == 5
    # so many ineligible that an update's q nearest include one: its score is +inf; fewer than m finite
    nf = np.array([0, 0, 1, 1, 1, 0, 0], np.int64)
    sc, sel = krum.select(gram, nf, None, 2, 5)                          # q = 3 = the 3 eligible others
    assert [math.isfinite(v) for v in sc] == [True, True, False, False, False, True, True] and sel == [0, 1, 5, 6]
    nf = np.array([0, 0, 1, 1, 1, 1, 0], np.int64)                      # only 2 eligible others: every score +inf
    sc, sel = krum.select(gram, nf, None, 2, 5)
    assert all(math.isinf(v) for v in sc) and sel == []


def test_all_ineligible_returns_none_with_the_base_untouched(cpu_engine):
    ups = _ups(7, numel=8)
    for u in ups:
        u["w"][3] = float("nan")
    for sort in ("fedavg", "fedadam"):
        opt = _opt(sort, krum=2)
        base = {"w": torch.ones(8), "nbt": torch.tensor(5)}
        cache = _cache(ups)
        res = opt.do(base, cache, total=7)
        assert res is None and len(cache) == 0
        assert torch.equal(base["w"], torch.ones(8)) and int(base["nbt"]) == 5 and cpu_engine["accumulate"] == []
        assert [r.selected for r in opt.krum_records] == [False] * 7 and all(r.nonfinite == 1 for r in opt.krum_records)


def test_guard_reads_the_gram_diagonal(cpu_engine):
    """clip_threshold with krum: the guard's records come from diag(G) and the counts, no second
    measuring pass (engine.update_stats raises here), and the clip scales reach the reduction."""
    from flame_amd.optimizer import guard
    n, f = 9, 2
    ups = _ups(n, numel=1023, seed=4, f=f)
    x = np.stack([R.flatten(u)[0] for u in ups])
    norms = [math.sqrt(float(v)) for v in (x @ x.T).diagonal()]      # the fixture's own Gram matrix
    clip = sorted(norms)[-2] * 0.5
    opt = _opt("fedavg", krum=f, clip_threshold=clip)
    base = {"w": torch.zeros(1023), "nbt": torch.tensor(0)}
    opt.do(base, _cache(ups), total=n)
    assert cpu_engine["stats"] == 0 and len(opt.update_stats) == n
    assert [r.scale for r in opt.update_stats] == [guard.clip_scale(x, clip) for x in norms]
    sel = [i for i, r in enumerate(opt.krum_records) if r.selected]
    assert sel == R.krum(ups, f, scales=[r.scale for r in opt.update_stats])[1]
    rates, scales = cpu_engine["accumulate"][-1]
    assert rates == [1.0 / len(sel)] * len(sel) and scales == [opt.update_stats[i].scale for i in sel]
    # skip shrinks n and re-checks 2f + 3; raise raises with the records
    ups[1]["w"][0] = float("inf")
    opt = _opt("fedavg", krum=f, nonfinite="skip")
    opt.do({"w": torch.zeros(1023), "nbt": torch.tensor(0)}, _cache(ups), total=n)
    assert [r.skipped for r in opt.update_stats] == [i == 1 for i in range(n)] and not opt.krum_records[1].selected
    with pytest.raises(ValueError, match=r"2f \+ 3"):
        _opt("fedavg", krum=f, nonfinite="skip").do({"w": torch.zeros(1023), "nbt": torch.tensor(0)}, _cache(ups[:7]), total=7)
    opt = _opt("fedavg", krum=f, nonfinite="raise")
    with pytest.raises(ValueError, match="e01"):
        opt.do({"w": torch.zeros(1023), "nbt": torch.tensor(0)}, _cache(ups), total=n)
    assert [r.nonfinite for r in opt.update_stats] == [int(i == 1) for i in range(n)]


def test_the_four_refusals():
    from flame_amd.optimizers import optimizer_provider as P
    from flame_amd.shard import ShardedOptimizer
    # with trim
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5})):
        with pytest.raises(NotImplementedError, match="Krum / Multi-Krum"):
            P.get(sort, krum=1, trim=1, **kw)
    # with defer / chain_defer
    for sort in ("fedavg", "fedadam", "fedyogi", "fedadagrad"):
        with pytest.raises(NotImplementedError, match="defer"):
            P.get(sort, krum=1, defer=True)
    # under the sharded wrapper: at construction, and from the key groups it passes
    with pytest.raises(NotImplementedError, match="Krum / Multi-Krum"):
        ShardedOptimizer(P.get("fedavg", krum=1))
    for sort in ("fedavg", "fedadam"):
        opt = P.get(sort, krum=1)
        cache = _cache(_ups(5))
        with pytest.raises(NotImplementedError, match="all-reduce"):
            opt.do({"w": torch.zeros(40), "nbt": torch.tensor(0)}, cache, total=5, flame_amd_key_groups=[["w"], ["nbt"]])
        assert cache.pops == [] and len(cache) == 5
    # more than gram_max_clients() updates: test_unusable_rounds_raise_before_a_pop
    for sort, kw in (("fedbuff", {}), ("feddyn", {"alpha": 0.1}), ("scaffold", {"k": 3})):
        with pytest.raises(TypeError, match="krum"):
            P.get(sort, krum=1, **kw)                                   # these do not take the kwarg
    with pytest.raises(ValueError):                                     # a bad value is a bad value before it is refused
        P.get("fedavg", krum=0.5, trim=1)
    assert P.get("fedadam", krum=None).krum is None and P.get("fedavg", trim=1, krum=None).trim == 1


def test_classes_for_direct_use():
    import flame_amd.optimizers as fo
    from flame_amd.optimizer import FedAvg, FedKrum, FedMultiKrum
    mk, k = FedMultiKrum(0.2), FedKrum(1)
    assert isinstance(mk, FedAvg) and mk.krum == 0.2 and mk.krum_select is None
    assert isinstance(k, FedMultiKrum) and k.krum == 1 and k.krum_select == 1
    assert FedMultiKrum(2, select=3, clip_threshold=1.0, nonfinite="skip").guarded
    with pytest.raises(TypeError):
        FedMultiKrum(None)
    with pytest.raises(TypeError):
        FedKrum()
    with pytest.raises(ValueError):
        FedMultiKrum(0.5)
    assert FedMultiKrum not in fo.DROP_INS.values() and FedKrum not in fo.DROP_INS.values()
    assert len(fo.DROP_INS) == 9


def test_defaults_run_no_new_code(monkeypatch):
    from flame_amd import engine

    def boom(*a, **k):
        raise AssertionError("called")
    monkeypatch.setattr(engine, "update_gram", boom)
    monkeypatch.setattr(engine, "gram_max_clients", boom)
    seen = []
    monkeypatch.setattr(engine, "accumulate", lambda agg, entries, **kw: seen.append([r for _, r in entries]))
    for sort, kw in (("fedavg", {}), ("fedprox", {"mu": 0.1}), ("fedgft", {"fair": "SP", "gamma": 0.5})):
        opt = _opt(sort, **kw)
        assert opt.krum is None and opt.krum_select is None
        opt.do({"w": torch.zeros(3)}, _cache([{"w": torch.ones(3)}, {"w": torch.ones(3)}], [1, 3]), total=4)
        assert seen[-1] == [0.25, 0.75] and opt.krum_records == []       # today's weighted path


def test_kwargs_resolve_from_a_job_optimizer_block():
    import flame_amd.optimizers as fo
    provider = fo.install(fo.OptimizerProvider())
    for block, want in (('{"sort": "fedavg", "kwargs": {"krum": 2}}', (2, None)),
                        ('{"sort": "fedadam", "kwargs": {"krum": 0.2, "clip_threshold": 1.0}}', (0.2, None)),
                        ('{"sort": "fedprox", "kwargs": {"mu": 0.01, "krum": 1, "krum_select": 1}}', (1, 1))):
        job = json.loads(block)
        o = provider.get(job["sort"], **job["kwargs"])
        assert (o.krum, o.krum_select) == want and type(o.krum) is type(want[0])
        assert o.do({}, S.SortedCache(), total=0) is None


def test_engine_refuses_on_the_host():
    """engine.update_gram's own checks that need no device."""
    from flame_amd import engine
    g, nf = engine.update_gram([])
    assert g.shape == (0, 0) and nf.shape == (0,)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            engine.update_gram([{"w": torch.ones(8)} for _ in range(3)])
