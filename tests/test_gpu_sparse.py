"""flame_sparse_index + flame_agg_reduce_sparse on the GPU, BITWISE against tests/sparse_ref.py: the shapes,
entry counts, edges and values at which the gather can go wrong; the bad-index refusals; the densified equivalence."""
import numpy as np
import pytest
import torch

import scenarios as S
import sparse_ref
from large_case import Launches

pytestmark = [pytest.mark.gpu]
DEV, SUB = "cuda:0", 1024
NUMELS = {"a": 1, "b": 1023, "c": 1024, "d": 1025, "e": 4097, "f": 3 * 4096 + 5}
COUNTS = (0, 1, 64, 65, 1024)      # entries per (client, sub-range): none, one, a full step, a step and one, dense
SPARE, HIT = 5, 7                   # element 5 of every key is never sent; every client sends element 7 of e and f


def _case(n):        # (base, updates): updates[c][key] = (int32 indices, fp32 values), numpy
    rng = np.random.default_rng(n)
    base = {k: rng.standard_normal(m).astype(np.float32) for k, m in NUMELS.items()}
    mags = np.float32(10.0) ** rng.permutation(np.linspace(-30, 30, n)).astype(np.float32)     # a wrong order changes bits
    ups = []
    for c in range(n):
        up, empty = {}, n >= 8 and c == 3                       # a client with nnz == 0
        for ki, (k, m) in enumerate(NUMELS.items()):
            idx = [HIT] if k in "ef" and not empty else []
            for s in range(-(-m // SUB)):
                lo, hi = s * SUB, min(m, (s + 1) * SUB)         # (sub-range 0 stays under 66 entries: SPARE is untouched)
                cnt = 0 if empty else min(COUNTS[(c + s + ki) % 5], hi - lo, 65 if s == 0 else SUB)
                edges = [lo, hi - 1] if cnt >= 2 else [hi - 1 if c % 2 else lo][:cnt]
                pool = np.setdiff1d(np.arange(lo, hi), edges + [SPARE, HIT])
                idx += edges + rng.choice(pool, max(0, min(cnt - len(edges), pool.size)), replace=False).tolist()
            idx = np.unique(np.asarray(idx, dtype=np.int32))
            val = (rng.standard_normal(idx.size) * 1e-2).astype(np.float32)
            val[idx == HIT] = mags[c] * (-1) ** c if k in "ef" else val[idx == HIT]
            if k == "d" and idx.size >= 3:
                val[:3] = (1.5e-38, np.inf, np.nan)             # a subnormal product, inf, NaN
            up[k] = (idx, val)
        ups.append(up)
    for k, m in NUMELS.items():
        base[k][SPARE:SPARE + 1] = -0.0
    base["d"][ups[0]["d"][0][0]] = 0.0                          # the subnormal product lands on a zero and stays
    return base, ups


def _dev(a, misalign=False):     # a on the device; misalign: as a view 4 bytes into its buffer (4-byte, not 16-byte aligned)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    buf[1:] = torch.from_numpy(a)
    return buf[1:] if misalign else buf[1:].clone()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", [1, 8, 9, 70])
def test_reduce_matches_the_contract(n, scaled):
    """Odd clients' index and value tensors are misaligned views; at n = 9 the aggregate is one too (FLAME_SEG_UNALIGNED)."""
    from flame_amd import engine, sparse
    base, ups = _case(n)
    rates = [(c + 1) / (n * (n + 1) / 2) for c in range(n)]
    scales = [1.0 if c % 3 else 1.0 / (c + 3) for c in range(n)] if scaled else None
    want = {k: torch.from_numpy(sparse_ref.accumulate(base[k], [u[k] for u in ups], rates, scales)) for k in base}
    ws = [sparse.SparseWeights({k: _dev(v, c % 2) for k, (_, v) in u.items()}, {k: _dev(i, c % 2) for k, (i, _) in u.items()},
                               {k: (NUMELS[k],) for k in u}) for c, u in enumerate(ups)]
    got = []
    for _ in range(2):
        agg = {k: _dev(v, n == 9) for k, v in base.items()}
        with Launches() as ln:
            engine.accumulate(agg, list(zip(ws, rates)), scales=scales)
        assert ln.names == ["flame_sparse_index", "flame_agg_reduce_sparse"], ln.names
        S.same_bits(f"sparse n={n}", agg, want)
        got.append(agg)
    assert all(torch.equal(got[0][k].view(torch.int32), got[1][k].view(torch.int32)) for k in base)      # equal launches, equal bits


@pytest.mark.parametrize("idx", [[3, 9, 8, 20], [3, 9, 9, 20], [-1, 9, 10, 20], [3, 9, 10, 5000]], ids=["unsorted", "duplicate", "negative", "numel"])
def test_bad_indices_raise_before_the_reduce(idx):
    from flame_amd import engine, sparse
    agg = {"w": torch.ones(5000, device=DEV), "d": torch.ones(9, device=DEV)}
    good, bad = (sparse.SparseWeights({"w": torch.ones(4), "d": torch.ones(9)}, {"w": torch.tensor(i, dtype=torch.int32)},
                                      {"w": (5000,)}).to(DEV) for i in ([0, 1, 2, 4999], idx))
    with Launches() as ln:
        with pytest.raises(ValueError, match=r"position\(s\) 1 \(1 bad entries\)"):
            engine.accumulate(agg, [(good, 0.5), (bad, 0.25), (good, 0.25)])
    assert ln.names == ["flame_sparse_index"] and all(bool((v == 1).all()) for v in agg.values()), ln.names


@pytest.mark.parametrize("sort,noise", [("accumulate", None), ("fedavg", None), ("fedavg", 0.01), ("fedprox", None), ("fedprox", 0.01)])
def test_equals_the_round_over_the_densified_updates(sort, noise):
    from flame_amd import engine, sparse
    from flame_amd.optimizers import optimizer_provider
    g = torch.Generator().manual_seed(11)
    model = {"w": torch.randn(3, 4099, generator=g), "b": torch.randn(77, generator=g), "n": torch.tensor(3)}
    ups = [sparse.topk({k: torch.randn(v.shape, generator=g).to(v.dtype) for k, v in model.items()}, ratio=0.03) for _ in range(4)]
    out = []
    for dense in (False, True):
        ws = [{k: v.to(DEV) for k, v in sparse.densify(u).items()} if dense else u.to(DEV) for u in ups]
        agg, cache = {k: v.to(DEV) for k, v in model.items()}, S.SortedCache()
        for i, w in enumerate(ws):
            cache[f"e{i}"] = S.TR(w, 2 + i, 0)
        if sort == "accumulate":
            engine.accumulate(agg, [(w, (2 + i) / 14) for i, w in enumerate(ws)])
        else:
            kw = {"mu": 0.1} if sort == "fedprox" else {}
            agg = optimizer_provider.get(sort, **kw, **({} if noise is None else {"noise_factor": noise, "noise_seed": 9})).do(agg, cache, total=14)
        out.append(agg)
    S.same_bits(f"{sort} sparse vs densify", out[0], {k: v.cpu() for k, v in out[1].items()})
