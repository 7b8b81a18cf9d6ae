"""The fp64 FedOPT entry points (flame_fedopt_reduce_adapt_f64, flame_fedopt_chain_f64) on the
host: the symbols resolve, invalid arguments are refused before any HIP call, the launch-branch
table grew by exactly the six appended fp64 branches (every earlier index and name kept), the
fp32-typed entry points still refuse FLAME_F64, and the drop-in's queue admits an fp64 model.
No GPU call."""
import ctypes

import pytest
import torch

DTS = ["f32", "bf16", "f16", "f64", "i64", "i32"]
F3 = DTS[:3]
VAR = ["fedadam", "fedyogi", "fedadagrad"]
MODE = ["fedbuff", "sync"]

# branch_name() of fedagg.hip for indices 0..93, in index order
FIRST_94 = (
    [f"flame_agg_reduce/{d}" for d in DTS]
    + [f"flame_agg_reduce/lo/{d}" for d in F3]
    + [f"flame_agg_reduce_argmeta/{d}" for d in DTS]
    + [f"flame_fedopt_reduce_adapt/{d}/{v}" for d in F3 for v in VAR]
    + [f"flame_fedopt_reduce_adapt/multi/f32/{v}" for v in VAR]
    + [f"flame_fedopt_reduce_adapt_argmeta/{d}/{v}" for d in F3 for v in VAR]
    + [f"flame_fedbuff_scale_add/{d}" for d in DTS[:4]]
    + [f"flame_hier_fedbuff/reg/{d}/{m}" for d in F3 for m in MODE]
    + [f"flame_hier_fedbuff/lds/{d}/{m}" for d in F3 for m in MODE]
    + [f"flame_hier_fedbuff/lo/{d}/fedbuff" for d in F3]
    + [f"flame_hier_fedbuff_argmeta/{d}/{m}" for d in F3 for m in MODE]
    + [f"flame_feddyn_round/{d}" for d in DTS[:4]]
    + [f"flame_agg_reduce_argmeta/lo_burst/{d}" for d in F3]
    + [f"flame_hier_fedbuff_argmeta/lo/{d}/fedbuff" for d in F3]
    + [f"flame_fedopt_reduce_adapt_argmeta/multi/f32/{v}" for v in VAR]
    + [f"flame_hier_fedbuff_argmeta/lds/{d}/{m}" for d in F3 for m in MODE]
    + [f"flame_fedopt_chain/{d}/{v}" for d in F3 for v in VAR]
    + [f"flame_agg_reduce/lo_burst/{d}" for d in F3]
    + ["flame_elementwise", "flame_elementwise_segments"]
)
NEW_6 = [f"flame_fedopt_reduce_adapt/f64/{v}" for v in VAR] + [f"flame_fedopt_chain/f64/{v}" for v in VAR]

HYPER = [0.9, 1 - 0.9, 0.99, 1 - 0.99, 1e-2, 1e-3]


def _lib():
    from flame_amd import _native
    return _native, _native.lib()


def test_symbols_resolve():
    N, L = _lib()
    assert L.flame_abi_version() == 1
    for name in ("flame_fedopt_reduce_adapt_f64", "flame_fedopt_chain_f64"):
        assert name in N.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int
        assert getattr(L, name).argtypes.count(ctypes.c_double) == 6


def test_reduce_adapt_f64_validates_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host

    def call(variant=0, flags=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, n_clients=1, rates=fake):
        return L.flame_fedopt_reduce_adapt_f64(variant, flags, segs, n_segs, n_chunks, clients, n_clients, rates,
                                               *HYPER, None)
    assert call(segs=None, n_segs=0) == N.FLAME_EINVAL
    assert b"segment" in L.flame_last_error()
    assert call(n_chunks=0) == N.FLAME_EINVAL
    assert call(clients=None) == N.FLAME_EINVAL
    assert call(rates=None) == N.FLAME_EINVAL                 # NULL rates with clients
    assert b"rate" in L.flame_last_error()
    assert call(variant=7) == N.FLAME_ENOTSUP
    assert b"variant" in L.flame_last_error()
    assert call(variant=-1) == N.FLAME_ENOTSUP
    assert call(flags=4) == N.FLAME_EINVAL
    assert b"unknown flags" in L.flame_last_error()


def test_chain_f64_validates_without_gpu():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: every call below fails on the host

    def call(variant=0, flags=0, segs=fake, n_segs=1, n_chunks=1, clients=fake, n_clients=1, rates=fake, ends=fake):
        return L.flame_fedopt_chain_f64(variant, flags, segs, n_segs, n_chunks, clients, n_clients, rates, ends,
                                        *HYPER, None)
    assert call(segs=None, n_segs=0) == N.FLAME_EINVAL
    assert call(clients=None, n_clients=0) == N.FLAME_EINVAL  # a chain needs at least one client
    assert b"client" in L.flame_last_error()
    assert call(rates=None) == N.FLAME_EINVAL
    assert call(ends=None) == N.FLAME_EINVAL
    assert b"step_end" in L.flame_last_error()
    assert call(variant=7) == N.FLAME_ENOTSUP
    assert call(flags=2) == N.FLAME_EINVAL                    # FLAME_OPT_XCD_MAP is not a chain flag
    assert b"unknown flags" in L.flame_last_error()


def test_launch_branch_table_appended():
    N, L = _lib()
    assert len(FIRST_94) == 94 and len(set(FIRST_94 + NEW_6)) == 100
    assert L.flame_launch_branches() == 100
    names = list(N.launch_branch_counts())
    assert names[:94] == FIRST_94
    assert names[94:] == NEW_6


def test_fp32_typed_entry_points_still_refuse_f64():
    N, L = _lib()
    fake = ctypes.c_void_p(4096)    # never dereferenced: the dtype is refused on the host
    f32 = [0.9, 0.1, 0.99, 0.01, 0.01, 0.001]
    assert L.flame_fedopt_reduce_adapt(N.FLAME_F64, 0, 0, fake, 1, 1, fake, 1, fake, *f32, None) == N.FLAME_ENOTSUP
    assert b"not supported" in L.flame_last_error()
    assert L.flame_fedopt_chain(N.FLAME_F64, 0, 0, fake, 1, 1, fake, 1, fake, fake, *f32, None) == N.FLAME_ENOTSUP
    assert b"not supported" in L.flame_last_error()


def test_scalars_carry_the_python_floats():
    """engine.fedopt_scalars: the fp32 roundings to every caller that unpacks it, the unrounded
    Python floats (what torch multiplies an fp64 tensor by) in .raw."""
    import pickle

    import numpy as np
    from flame_amd import engine
    h = engine.fedopt_scalars(0.9, 0.99, 1e-2, 1e-3)
    f = np.float32
    assert tuple(h) == (f(0.9), f(1 - 0.9), f(0.99), f(1 - 0.99), f(1e-2), f(1e-3)) and len(h) == 6
    assert all(isinstance(x, np.float32) for x in h)
    assert h.raw == (0.9, 1 - 0.9, 0.99, 1 - 0.99, 1e-2, 1e-3)
    assert h.raw[1] != float(h[1])                 # 1 - beta_1 never passes through fp32
    assert engine._scalars64(h) == list(h.raw)
    q = pickle.loads(pickle.dumps(h))
    assert tuple(q) == tuple(h) and q.raw == h.raw
    with pytest.raises(TypeError):
        engine._scalars64(tuple(h))


class TR:
    def __init__(self, weights, count):
        self.weights, self.count, self.version = weights, count, 0


class Cache(dict):
    def iterkeys(self):
        return iter(sorted(self))


@pytest.mark.parametrize("dtypes", [(torch.float64,), (torch.float32, torch.float64)], ids=["f64", "f32+f64"])
def test_deferred_queue_admits_fp64(monkeypatch, dtypes):
    """FedAdam(defer=True) queues an fp64 (or mixed f32 + f64) model: float64 is a chain dtype,
    _try_queue returns a DeferredCurrent, the queue's byte estimate uses the element size, and
    the flush hands fedopt_chain_ the fp64 tensors with scalars that carry .raw."""
    from flame_amd import engine
    from flame_amd.optimizer import fedopt as F
    from flame_amd.optimizers import optimizer_provider
    assert torch.float64 in F._CHAIN_DTYPES
    assert set(F._CHAIN_DTYPES) == {torch.float32, torch.bfloat16, torch.float16, torch.float64}
    # the eligibility rule with its device test taken out (no GPU here); the dtype rule is the module's own
    monkeypatch.setattr(F, "_chain_tensors", lambda w: all(t.dtype in F._CHAIN_DTYPES and t.is_contiguous()
                                                            for t in w.values()))
    seen = []

    def fake_chain(variant, base, cur, cur_out, m, v, clients, rates, step_end, hyper, state_zero, first_aliased):
        seen.append(([b.dtype for b in base], hyper.raw, list(rates), list(step_end)))
        for b, o, mm, vv in zip(base, cur_out, m, v):
            o.copy_(b + 1)
            mm.fill_(0.5)
            vv.fill_(0.25)
    monkeypatch.setattr(engine, "fedopt_chain_", fake_chain)
    opt = optimizer_provider.get("fedadam", defer=True)
    base = {f"k{i}": torch.zeros(8 + i, dtype=dt) for i, dt in enumerate(dtypes)}
    opt._current = base                 # the state right after round 1's passthrough (current IS base)
    res = None
    for i in (1, 2):
        c = Cache()
        c[f"e{i}"] = TR({k: torch.full_like(t, float(i)) for k, t in base.items()}, 5)
        res = opt.do(base, c, total=10)
        assert isinstance(res, F.DeferredCurrent) and not seen
    assert opt._chain.nbytes == 2 * sum(t.numel() * t.element_size() for t in base.values())
    out = dict(res)
    assert [t.dtype for t in out.values()] == list(dtypes)
    assert len(seen) == 1 and seen[0][0] == list(dtypes)
    assert seen[0][1] == (0.9, 1 - 0.9, 0.99, 1 - 0.99, 1e-2, 1e-3) and seen[0][2] == [0.5, 0.5]
    assert seen[0][3] == [True, True]
