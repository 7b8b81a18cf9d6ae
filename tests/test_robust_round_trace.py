"""The update guard, ``trim`` and ``krum`` across classes and combinations, without a GPU.

tests/test_update_guard_host.py, test_trimmed_host.py and test_krum_host.py each pin one feature.
Here one table walks what the optimizers' selection stage owns as a whole: every class that takes
the kwargs x every mode below, three rounds each over the same seven tiny CPU updates (one holds a
NaN, one has a large norm), with the engine's entry points and the metric collector replaced by
recorders.  Per round the trace holds the ordered engine calls (number of updates, rates, scales),
the cache's pop order and what is left of it, what ``do()`` returned, ``update_stats``,
``krum_records``, ``trim_k``, every metric saved and the exception, if any; a combination refused at
construction is its exception.  Floats are ``float.hex()``.

The expected traces are ``tests/golden/robust_round_trace.json``, written by
``tests/golden/make_robust_round_trace.py`` from the optimizers as they stood before the four
pop / measure / decide helpers were merged into one stage; the comparison is for equality.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import scenarios as S

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robust_round_trace.json")
CLIP = 5.0
CLASSES = {"fedavg": {}, "fedprox": {"mu": 0.1}, "fedgft": {"fair": "SP", "gamma": 0.5}, "fedadam": {}}
MODES = {
    "plain": {},
    "clip": {"clip_threshold": CLIP},
    "skip": {"nonfinite": "skip"},
    "raise": {"nonfinite": "raise"},
    "clip_skip": {"clip_threshold": CLIP, "nonfinite": "skip"},
    "trim": {"trim": 1},
    "trim_skip": {"trim": 1, "nonfinite": "skip"},
    "krum": {"krum": 1},
    "krum_clip": {"krum": 1, "clip_threshold": CLIP},
    "krum_skip": {"krum": 1, "nonfinite": "skip"},
    "krum_skip_empties": {"krum": 1, "nonfinite": "skip"},      # after the first round every update holds a NaN
}
ROUNDS, N_UPDATES, NAN_AT, LARGE_AT = 3, 7, 2, 5
COUNTS = [3, 1, 4, 1, 5, 9, 2]


def enc(x):
    """JSON-able, exact: floats as hex, tuples (records among them) as lists."""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, (list, tuple)):
        return [enc(v) for v in x]
    raise TypeError(f"untraceable value {x!r}")


def _updates(all_nan=False):
    # multiples of 1/8 from a fixed recurrence: exact in fp32, the same on every machine
    vals = iter([((37 * i * i + 11 * i) % 29 - 14) / 8.0 for i in range(9 * N_UPDATES)])
    ups = [{"w": torch.tensor([next(vals) for _ in range(6)]), "b": torch.tensor([next(vals) for _ in range(3)])}
           for _ in range(N_UPDATES)]
    ups[LARGE_AT]["w"] *= 100.0
    for i, u in enumerate(ups):
        if all_nan or i == NAN_AT:
            u["b"][1] = float("nan")
    return ups


class CountingCache(S.SortedCache):
    def __init__(self, ups):
        super().__init__()
        self.pops = []
        for i, (u, c) in enumerate(zip(ups, COUNTS)):
            self[f"e{i}"] = S.TR(u, c)

    def pop(self, k, default=None):
        self.pops.append(k)
        return super().pop(k, default)


class Collector:
    def __init__(self, log):
        self.log = log

    def save(self, mtype, alias, value):
        self.log.append([mtype, alias, enc(value)])


def _flat(w):
    """An update's float elements as Python floats, the non-finite ones as 0.0, and their count."""
    x = [float(v) for k in w.keys() for v in w[k].double().reshape(-1)]
    return [v if math.isfinite(v) else 0.0 for v in x], sum(not math.isfinite(v) for v in x)


def _dot(x, y):
    return math.fsum(a * b for a, b in zip(x, y))      # correctly rounded: no summation order to depend on


def _fakes(monkeypatch, calls):
    """Recorders for every engine entry point a round can reach (none computes an aggregate: the
    trace holds what the optimizers decide, not the arithmetic the GPU suites pin)."""
    from flame_amd import engine

    def update_stats(ws, device=None):
        flat = [_flat(w) for w in ws]
        calls.append(["update_stats", len(flat)])
        return np.asarray([_dot(x, x) for x, _ in flat], np.float64), np.asarray([b for _, b in flat], np.int64)

    def update_gram(ws, device=None):
        flat = [_flat(w) for w in ws]
        calls.append(["update_gram", len(flat)])
        gram = np.asarray([[_dot(x, y) for y, _ in flat] for x, _ in flat], np.float64)
        return gram, np.asarray([b for _, b in flat], np.int64)

    def accumulate(agg, entries, **kw):
        calls.append(["accumulate", len(entries), enc([r for _, r in entries]), enc(kw.get("scales")),
                      sorted(k for k, v in kw.items() if v is not None)])

    def trimmed_mean(agg, ws, k, *, init_first=False, device=None):
        calls.append(["trimmed_mean", len(list(ws)), k, init_first])

    def reduce_(outs, ins, clients, rates, **kw):
        calls.append(["reduce_", [len(c) for c in clients], enc(list(rates)), enc(kw.get("scales"))])

    def fedopt_reduce_adapt_(variant, avg_out, base, cur, cur_out, m, v, clients, rates, hyper, state_zero, **kw):
        calls.append(["fedopt_reduce_adapt_", variant, [len(c) for c in clients], enc(list(rates)), bool(state_zero)])

    for name, fn in (("update_stats", update_stats), ("update_gram", update_gram), ("accumulate", accumulate),
                     ("trimmed_mean", trimmed_mean), ("reduce_", reduce_), ("fedopt_reduce_adapt_", fedopt_reduce_adapt_),
                     ("gram_max_clients", lambda: 1024), ("trimmed_max_k", lambda: 16),
                     ("pick_device", lambda *a: torch.device("cpu"))):
        monkeypatch.setattr(engine, name, fn)
    monkeypatch.setattr(engine._Target, "__init__",
                        lambda self, t, device: (setattr(self, "orig", t), setattr(self, "dev", t))[0])


def run_case(sort, mode, monkeypatch):
    """The trace of one class in one mode: ``{"construct": [...]}`` or ``{"rounds": [...]}``."""
    from flame_amd.optimizers import optimizer_provider
    calls, saved = [], []
    _fakes(monkeypatch, calls)
    try:
        opt = optimizer_provider.get(sort, **CLASSES[sort], **MODES[mode])
    except Exception as e:  # noqa: BLE001 - the refusal is the trace
        return {"construct": [type(e).__name__, str(e)]}
    opt.metric_collector = Collector(saved)
    base = {"w": torch.zeros(6), "b": torch.zeros(3)}
    rounds = []
    for r in range(ROUNDS):
        del calls[:], saved[:]
        cache = CountingCache(_updates(all_nan=mode == "krum_skip_empties" and r > 0))
        rec = {"exception": None, "returned": None}
        try:
            out = opt.do(base, cache, total=sum(COUNTS))
            rec["returned"] = ("none" if out is None else "base" if out is base else
                               "current_weights" if out is getattr(opt, "current_weights", None) else type(out).__name__)
        except Exception as e:  # noqa: BLE001 - the exception is part of the trace
            rec["exception"] = [type(e).__name__, str(e)]
        rec.update(calls=list(calls), pops=list(cache.pops), left=len(cache), update_stats=enc(opt.update_stats),
                   krum_records=enc(opt.krum_records), trim_k=opt.trim_k, metrics=list(saved),
                   agg_weights="none" if opt.agg_weights is None else "base" if opt.agg_weights is base else "other")
        rounds.append(rec)
    return json.loads(json.dumps({"rounds": rounds}))


def _expected():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_the_table():
    assert sorted(_expected()) == sorted(f"{s}-{m}" for s in CLASSES for m in MODES)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("sort", list(CLASSES))
def test_round_trace(sort, mode, monkeypatch):
    got, exp = run_case(sort, mode, monkeypatch), _expected()[f"{sort}-{mode}"]
    assert list(got) == list(exp)
    if "rounds" in exp:
        for i, (g, e) in enumerate(zip(got["rounds"], exp["rounds"])):
            for field in e:
                assert g[field] == e[field], f"{sort}-{mode}: round {i}: {field} differs"
    assert got == exp


def test_the_table_reaches_every_branch():
    """The fixture itself: every mode does what its name says somewhere in the table."""
    exp = _expected()
    first = lambda key: exp[key]["rounds"][0]     # noqa: E731
    assert [c[0] for c in first("fedavg-plain")["calls"]] == ["accumulate"] and first("fedavg-plain")["update_stats"] == []
    assert first("fedavg-clip")["calls"][1][3] is not None and first("fedavg-skip")["calls"][1][3] is None
    assert first("fedavg-skip")["calls"][1][1] == N_UPDATES - 1 and first("fedavg-raise")["exception"][0] == "NonFiniteUpdate"
    assert first("fedavg-raise")["left"] == 0 and len(first("fedavg-raise")["update_stats"]) == N_UPDATES
    assert [c[0] for c in first("fedavg-trim_skip")["calls"]] == ["update_stats", "trimmed_mean"]
    assert [c[0] for c in first("fedavg-krum_clip")["calls"]] == ["update_gram", "accumulate"]
    emptied = exp["fedavg-krum_skip_empties"]["rounds"][1]
    assert emptied["returned"] == "none" and emptied["left"] == 0 and emptied["calls"] == [["update_gram", N_UPDATES]]
    assert "construct" in exp["fedadam-trim"] and "construct" in exp["fedadam-trim_skip"]
    adam = exp["fedadam-krum_clip"]["rounds"]
    assert [c[0] for c in adam[0]["calls"]] == ["update_gram", "accumulate"]
    assert [c[0] for c in adam[1]["calls"]] == ["update_gram", "reduce_", "fedopt_reduce_adapt_"]
    assert [c[0] for c in exp["fedadam-plain"]["rounds"][2]["calls"]] == ["fedopt_reduce_adapt_"]
    # the fused round: current_weights (after the first round's passthrough, the base dict), no aggregate
    emptied = exp["fedadam-krum_skip_empties"]["rounds"][1]
    assert emptied["returned"] == "base" and emptied["agg_weights"] == "none" and len(emptied["calls"]) == 1
