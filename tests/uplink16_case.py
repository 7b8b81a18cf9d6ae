"""Shared pieces of the 16-bit-uplink tests: the torch-CPU restatement of the reference's two
statements (fedavg.py:93-104, with differential_privacy.py:79-82 in front when clipped) and the
drivers that replay tests/golden/uplink16.npz through any optimizer implementation."""
from copy import deepcopy

import torch

import scenarios as S

SORTS = ("fedadam", "fedyogi", "fedadagrad")


def restate(base, clients, rates, scales=None):
    """``tmp = v * rate; base += tmp`` per client in order, on torch-CPU: tmp in v's dtype, the add
    in the promoted one.  ``scales``: ``v = torch.mul(v, scale)`` first."""
    out = base.clone()
    for i, (v, r) in enumerate(zip(clients, rates)):
        if scales is not None:
            v = torch.mul(v, scales[i])
        tmp = v * r
        tmp = tmp.to(dtype=v.dtype) if tmp.dtype != v.dtype else tmp
        out += tmp
    return out


def run_fedavg(fx, prefix, make_opt, device, wrap=None):
    """The sync FedAvg case under ``prefix``: [(label, got, expected)].  ``wrap(weights, i)`` turns
    client i's CPU weights into what the cache holds (default: copies on ``device``)."""
    m = fx.meta[prefix]
    base = S.to_dev(fx.weights(f"{prefix}/base"), device)
    cache = S.SortedCache()
    for i, (e, c) in enumerate(zip(m["end_ids"], m["counts"])):
        w = fx.weights(f"{prefix}/client{i}")
        cache[e] = S.TR(S.to_dev(w, device) if wrap is None else wrap(w, i), c)
    assert list(cache.iterkeys()) == m["order"]
    out = make_opt("fedavg").do(base, cache, total=m["total"], num_trainers=m["n"])
    assert out is base and len(cache) == 0
    return [(f"{prefix}/out", out, fx.weights(f"{prefix}/out"))]


def run_fedopt(fx, sort, make_opt, device, each_round=None):
    """The three sync rounds of ``sort``: [(label, got, expected)] with labels r<k>/<what>."""
    m = fx.meta[sort]
    opt = make_opt(sort, beta_1=m["beta_1"], beta_2=m["beta_2"], eta=m["eta"], tau=m["tau"])
    weights = S.to_dev(fx.weights(f"{sort}/weights0"), device)
    res = []
    for r in range(m["rounds"]):
        cache = S.SortedCache()
        for i, c in enumerate(m["counts"][r]):
            cache[f"r{r}c{i}"] = S.TR(S.to_dev(fx.weights(f"{sort}/r{r}/client{i}"), device), c)
        weights = opt.do(deepcopy(weights), cache, total=sum(m["counts"][r]), num_trainers=m["n"])
        res.append((f"r{r}/cur", S.to_cpu(weights), fx.weights(f"{sort}/r{r}/cur")))
        res.append((f"r{r}/avg", S.to_cpu(opt.agg_weights), fx.weights(f"{sort}/r{r}/avg")))
        if f"{sort}/r{r}/m" in fx.meta["keys"]:
            res.append((f"r{r}/m", S.to_cpu(opt.m_t), fx.weights(f"{sort}/r{r}/m")))
            res.append((f"r{r}/v", S.to_cpu(opt.v_t), fx.weights(f"{sort}/r{r}/v")))
        if each_round is not None:
            each_round(r, opt)
    return res


def check_fedopt(name, res):
    """The contract of the fp32 FedOPT fixtures (tests/test_oracle_golden.py): FedAvg arithmetic
    bitwise, the adaptive step within SURVEY §8(c)."""
    for label, got, exp in res:
        rnd = int(label.split("/")[0][1:])
        if label in ("r0/cur", "r0/avg", "r1/avg"):
            S.assert_bitwise(f"{name}:{label}", got, exp)
        else:
            S.assert_close_fedopt(f"{name}:{label}", got, exp, elementwise=rnd <= 1)
