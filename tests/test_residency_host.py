"""Where tensors live, on the host (no GPU: the launches are replaced by recorders).

INTEGRATION.md documents a host-resident model, pinned updates and checkpoint-restored (host)
optimizer state as supported.  A host pointer that reaches a kernel unstaged is a GPU memory fault,
so the plumbing that decides residency is pinned here, before tests/test_gpu_residency.py runs it
for real:

* FedOPT's generic keys (an int64 ``num_batches_tracked``) run their flame_elementwise program on
  the round's compute device, not on the device the FedAvg result happens to live on;
* ``elementwise.materialize`` / ``Program.__call__`` / ``Program.run_many`` refuse a non-GPU device
  by name before they allocate or launch;
* optimizer state a kernel writes, or whose address goes into a segment as it is, is staged
  (``engine._staged``), never handed on zero-copy; ``engine._as_device`` keeps its zero-copy
  contract for pinned updates.
"""
import types

import pytest
import torch

from flame_amd import _native as N
from flame_amd import elementwise as ew, engine
from flame_amd.optimizer import fedopt as F
from flame_amd.optimizers import optimizer_provider

GPU = torch.device("cuda", 0)


class TR:
    def __init__(self, weights, count):
        self.weights, self.count, self.version = weights, count, 0


class Cache(dict):
    def iterkeys(self):
        return iter(sorted(self))


def _model():
    return {"w": torch.arange(8, dtype=torch.float32), "nbt": torch.tensor(3, dtype=torch.int64),
            "d": torch.arange(4, dtype=torch.float64)}


def _cache(r):
    c = Cache()
    for i in range(2):
        c[f"r{r}e{i}"] = TR({"w": torch.full((8,), float(i)), "nbt": torch.tensor(100 + 37 * i),
                             "d": torch.full((4,), float(i), dtype=torch.float64)}, 1 + i)
    return c


@pytest.mark.parametrize("sort", ["fedadam", "fedyogi", "fedadagrad"])
def test_fedopt_generic_keys_run_on_the_compute_device(monkeypatch, sort):
    """A CPU base with an int64 0-dim key: from the first adaptive round on, every elementwise
    program of the generic keys is handed the device engine.pick_device chose."""
    recorded, fused_keys = [], []
    monkeypatch.setattr(engine, "pick_device", lambda *dicts: GPU)
    monkeypatch.setattr(engine, "accumulate", lambda agg, entries, **kw: None)

    def launch_fused(self, ks, base_weights, current, entries, device, hyper, state_zero, alloc, new_cur, scales=None):
        assert device == GPU
        fused_keys.append(list(ks))
        for k in ks:
            if state_zero:
                self.m_t[k], self.v_t[k] = torch.zeros_like(base_weights[k]), torch.zeros_like(base_weights[k])
            new_cur[k] = base_weights[k].clone()
    monkeypatch.setattr(F.FedOPT, "_launch_fused", launch_fused)

    def outputs(prog, row):
        return [torch.zeros(row[0].shape, dtype=dt) for dt in prog.out_dtypes]

    def run_many(self, rows, device, into=None):
        recorded.append(("run_many", device))
        return [outputs(self, row) for row in rows]

    def call(self, *inputs, device):
        recorded.append(("__call__", device))
        return outputs(self, inputs)
    monkeypatch.setattr(ew.Program, "run_many", run_many)
    monkeypatch.setattr(ew.Program, "__call__", call)

    opt = optimizer_provider.get(sort)
    base = _model()
    assert all(t.device.type == "cpu" for t in base.values())
    out = opt.do(base, _cache(0), total=3)
    assert out is base and recorded == []                 # round 1: the passthrough
    out = opt.do(base, _cache(1), total=3)                # current IS base (the eager caller's alias)
    assert recorded, "the generic keys launched nothing"
    assert fused_keys[-1] == ["w", "d"]
    # round 3: state from round 2; a fresh int64 counter keeps the key on the generic path
    out = opt.do({**{k: v.clone() for k, v in out.items()}, "nbt": torch.tensor(5)}, _cache(2), total=3)
    assert len(recorded) >= 2
    for what, device in recorded:
        assert device == GPU, f"Program.{what} was handed {device!r}, engine.pick_device chose {GPU!r}"
    # the new current of a generic key is the program's output (promoted to fp32), like m_t / v_t
    assert out["nbt"].dtype == torch.float32 and set(opt.m_t) == set(opt.v_t) == {"w", "nbt", "d"}


def test_elementwise_launch_sites_refuse_a_cpu_device(monkeypatch):
    def reached(*a, **k):
        raise AssertionError("a refused launch reached the library")
    monkeypatch.setattr(N, "lib", reached)
    monkeypatch.setattr(engine, "_launch", reached)
    x = torch.ones(3)
    prog = ew.trace(lambda a: a + 1, [(torch.float32, (3,))])
    for device in ("cpu", torch.device("cpu")):
        with pytest.raises(RuntimeError, match=r"elementwise\.materialize: tensors must live on the GPU, not on cpu"):
            ew.materialize(ew.Lazy.of(x) + 1, device=device)
        with pytest.raises(RuntimeError, match=r"elementwise\.materialize: .* not on cpu"):
            ew.materialize(ew.Lazy.of(x) + 1, device=device, into=[torch.empty(3)])
        with pytest.raises(RuntimeError, match=r"Program\.__call__: tensors must live on the GPU, not on cpu"):
            prog(x, device=device)
        with pytest.raises(RuntimeError, match=r"Program\.run_many: tensors must live on the GPU, not on cpu"):
            prog.run_many([[x], [x]], device)
        with pytest.raises(RuntimeError, match=r"Program\.run_many: .* not on cpu"):
            prog.run_many([[x]], device, into=[[torch.empty(3)]])
    with pytest.raises(RuntimeError, match="not on meta"):
        prog(x, device="meta")


class _Pinned:
    """A pinned host tensor as the staging helpers see it; ``to`` hands back a stand-in on the
    target device instead of copying (there is no GPU here)."""

    is_cuda = False

    def __init__(self, device=torch.device("cpu"), pinned=True, contiguous=True):
        self.device, self._pinned, self._contiguous, self.moves = device, pinned, contiguous, []

    def is_pinned(self):
        return self._pinned

    def is_contiguous(self):
        return self._contiguous

    def contiguous(self):
        return self if self._contiguous else _Pinned(self.device, self._pinned)

    def numel(self):
        return 4

    def data_ptr(self):
        return 0x1000

    def to(self, device, non_blocking=False):
        self.moves.append(device)
        return _Pinned(device, pinned=False)


def test_staged_never_takes_the_zero_copy_branch(monkeypatch):
    monkeypatch.setattr(engine, "ZERO_COPY_PINNED", True)
    t = _Pinned()
    same = engine._as_device(t, GPU)
    assert same is t and t.moves == []                    # updates: zero-copy, the contract stands
    s = engine._staged(t, GPU)
    assert s is not t and s.device == GPU and t.moves == [GPU]
    on_dev = _Pinned(GPU, pinned=False)
    assert engine._staged(on_dev, GPU) is on_dev and on_dev.moves == []
    strided = _Pinned(GPU, pinned=False, contiguous=False)
    assert engine._staged(strided, GPU).is_contiguous()
    pageable = _Pinned(pinned=False)
    assert engine._as_device(pageable, GPU).device == GPU and engine._staged(pageable, GPU).device == GPU


def _no_zero_copy(monkeypatch):
    staged = []

    def rec(t, device):
        staged.append(t)
        return t
    monkeypatch.setattr(engine, "_staged", rec)

    def refuse(t, device):
        raise AssertionError("optimizer state went through _as_device (its zero-copy branch)")
    monkeypatch.setattr(engine, "_as_device", refuse)
    return staged


def test_fedopt_fused_launch_stages_its_state(monkeypatch):
    """current / m_t / v_t of a fused key reach the launch through engine._staged."""
    staged = _no_zero_copy(monkeypatch)
    monkeypatch.setattr(engine, "_Target", lambda t, device: types.SimpleNamespace(orig=t, dev=t, writeback=lambda: None))
    seen = {}

    def reduce_adapt(variant, avg_out, base, cur, cur_out, m, v, clients, rates, hyper, state_zero, cur_is_avg=None):
        seen.update(cur=cur, m=m, v=v, alias=cur_is_avg)
    monkeypatch.setattr(engine, "fedopt_reduce_adapt_", reduce_adapt)
    opt = optimizer_provider.get("fedadam")
    base = {"w": torch.zeros(8), "a": torch.zeros(8)}
    current = {"w": torch.ones(8), "a": base["a"]}        # "a": the passthrough's alias (cur = avg)
    opt._m = {k: torch.zeros(8) for k in base}
    opt._v = {k: torch.zeros(8) for k in base}
    m0, v0 = dict(opt._m), dict(opt._v)
    new_cur = {}
    opt._launch_fused(["w", "a"], base, current, [({k: torch.ones(8) for k in base}, 1.0)], GPU,
                      engine.fedopt_scalars(0.9, 0.99, 1e-2, 1e-3), False,
                      lambda k, dt, shape: torch.empty(shape, dtype=dt), new_cur)
    want = [current["w"], m0["w"], v0["w"], m0["a"], v0["a"]]
    assert len(staged) == len(want) and all(any(s is w for s in staged) for w in want)
    assert seen["alias"] == [False, True] and seen["cur"][0] is current["w"] and seen["cur"][1] is base["a"]
    assert set(new_cur) == {"w", "a"}


def test_scale_add_stages_its_aggregate(monkeypatch):
    """FedBuff's aggregate goes into the segment by address: staged, not zero-copy."""
    staged = _no_zero_copy(monkeypatch)
    launches = []
    monkeypatch.setattr(engine, "_launch", lambda name, *a, **k: launches.append(name))
    monkeypatch.setattr(engine, "_keepalive", lambda keep, device: None)
    base, agg = torch.zeros(8), torch.ones(8)
    engine.scale_add_([base], [agg], 4)
    assert len(staged) == 1 and staged[0] is agg and launches == ["flame_fedbuff_scale_add"]
