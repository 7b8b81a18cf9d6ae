"""Generate tests/golden/uplink16.npz by running the REAL reference optimizers over bf16 / f16
updates into an fp32 model (a trainer that halves its uplink; fedavg.py:93-104 forms ``tmp`` in
the update's dtype and torch adds it in the promoted fp32).

Run in the build container only (the reference never travels), as make_golden.py is:

    PYTHONPATH=tests/golden/_shim:/root/reference/lib/python PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/make_golden_uplink16.py

Contents (prefixes of one fixture):
  fedavg/   sync FedAvg, 9 clients: fp32 base keys of 77 / 2,048 / 4,099 elements, one set with bf16
            and one with f16 client tensors
  model/    sync FedAvg, 9 clients, a BatchNorm-like model: two fp32 keys with bf16 updates, one fp32
            key with fp32 updates, an int64 num_batches_tracked
  fedadam/ fedyogi/ fedadagrad/   three sync rounds each, fp32 model, bf16 updates
"""
from __future__ import annotations

import os
import sys
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fixture_io import FixtureWriter  # noqa: E402

from flame.optimizers import optimizer_provider  # noqa: E402  (reference, via PYTHONPATH)
from flame.optimizer.train_result import TrainResult  # noqa: E402
from diskcache import Cache  # noqa: E402  (shim)

torch.set_num_threads(1)
HYPER = {"beta_1": 0.9, "beta_2": 0.99, "eta": 1e-2, "tau": 1e-3}


def weights(gen, spec, scale):
    out = {}
    for k, (shape, dt) in spec.items():
        if dt == torch.int64:
            out[k] = torch.randint(0, 50, shape, generator=gen, dtype=dt)
        else:
            out[k] = (torch.randn(shape, generator=gen, dtype=torch.float64) * scale).to(dt)
    return out


def fedavg(fw, prefix, base_spec, client_spec, n, seed):
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    base = weights(gen, base_spec, 1.0)
    clients = [weights(gen, client_spec, 1e-2) for _ in range(n)]
    ids = ["".join(rng.choice(list("0123456789abcdef"), 40)) for _ in range(n)]
    counts = [int(x) for x in rng.integers(1, 1001, n)]
    cache = Cache()
    for e, w, c in zip(ids, clients, counts):
        cache[e] = TrainResult(w, c)
    order = list(cache.iterkeys())
    out = optimizer_provider.get("fedavg").do(deepcopy(base), cache, total=sum(counts), num_trainers=n)
    for k, (_, dt) in base_spec.items():
        assert out[k].dtype == dt, (k, out[k].dtype)
    fw.meta[prefix] = {"n": n, "end_ids": ids, "counts": counts, "order": order, "total": sum(counts)}
    fw.put_weights(f"{prefix}/base", base)
    for i, w in enumerate(clients):
        fw.put_weights(f"{prefix}/client{i}", w)
    fw.put_weights(f"{prefix}/out", out)


def fedopt(fw, sort, seed):
    gen = torch.Generator().manual_seed(seed)
    spec = {"w": ((300,), torch.float32), "b": ((9,), torch.float32)}
    up = {k: (s, torch.bfloat16) for k, (s, _) in spec.items()}
    cur = weights(gen, spec, 1.0)
    opt = optimizer_provider.get(sort, **HYPER)
    n, rounds = 5, 3
    fw.put_weights(f"{sort}/weights0", cur)
    all_counts = []
    for r in range(rounds):
        clients = [weights(gen, up, 1e-2) for _ in range(n)]
        counts = [int(x) for x in torch.randint(1, 1001, (n,), generator=gen)]
        all_counts.append(counts)
        cache = Cache()
        for i, (w, c) in enumerate(zip(clients, counts)):
            cache[f"r{r}c{i}"] = TrainResult(w, c)
        cur = opt.do(deepcopy(cur), cache, total=sum(counts), num_trainers=n)
        for i, w in enumerate(clients):
            fw.put_weights(f"{sort}/r{r}/client{i}", w)
        fw.put_weights(f"{sort}/r{r}/avg", opt.agg_weights)
        fw.put_weights(f"{sort}/r{r}/cur", cur)
        if opt.m_t is not None:
            assert all(t.dtype == torch.float32 for t in list(opt.m_t.values()) + list(opt.v_t.values()))
            fw.put_weights(f"{sort}/r{r}/m", opt.m_t)
            fw.put_weights(f"{sort}/r{r}/v", opt.v_t)
    fw.meta[sort] = {"sort": sort, "n": n, "rounds": rounds, "counts": all_counts, **HYPER}


def main():
    fw = FixtureWriter()
    f32, bf, h = torch.float32, torch.bfloat16, torch.float16
    sizes = (77, 2048, 4099)
    base = {f"{p}{n}": ((n,), f32) for p in ("bf", "h") for n in sizes}
    cl = {f"{p}{n}": ((n,), dt) for p, dt in (("bf", bf), ("h", h)) for n in sizes}
    fedavg(fw, "fedavg", base, cl, 9, 1601)
    model = {"w1": ((2049,), f32), "w2": ((7, 11), f32), "f": ((33,), f32), "nbt": ((), torch.int64)}
    fedavg(fw, "model", model, {"w1": ((2049,), bf), "w2": ((7, 11), bf), "f": ((33,), f32), "nbt": ((), torch.int64)},
           9, 1602)
    for sort, seed in (("fedadam", 1611), ("fedyogi", 1612), ("fedadagrad", 1613)):
        fedopt(fw, sort, seed)
    fw.meta["kind"] = "uplink16"
    path = os.path.join(HERE, "uplink16.npz")
    fw.save(path)
    print("wrote uplink16.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
