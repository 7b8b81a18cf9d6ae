#!/usr/bin/env python3
"""What the top-k selection and the sparse downlink cost, in ONE process after the bench's HBM settling, the arms
alternating.

Arm 1, the selection alone: ``engine.topk`` (one flame_topk_select call: ten launches, five reads of the source)
against ``sparse.topk`` (``torch.topk`` plus a sort, the route it replaces) on the same device tensor of
``--params`` fp32 parameters, at ratios 0.1 %, 1 % and 10 %; device events around each call, medians over
``--rounds`` rounds with min and max, and for the native arm the call's own events as well (the kernels without
the launcher).  Beside it stands the same process's streaming-copy probe for the bytes of five reads: the rate of
``dst.copy_(src)`` over an fp32 tensor of that size, read plus written bytes.

Arm 2, the message: ``MessageEncoder.encode`` of ``{"weights": {"model": w}, "round": r}`` plain, with
``mx="e2m1"`` and with ``sparse=0.01`` (the weights move between messages, outside the clock); ``encode`` ends in
a synchronise, so a host clock around it is valid.  Payload sizes are recorded.

Every arm's output is checked against the contract ("the top-k selection") before its time counts.

    python tools/topk_rate.py                    # 25M parameters: the README's 100 MB model
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIOS = (0.001, 0.01, 0.1)


def _check(got, x, k):
    """``got`` (a SparseWeights on the device) is a selection of the contract for the flat fp32 tensor ``x``: k
    ascending indices, the values at them, no unselected magnitude above a selected one, and among the magnitudes
    equal to the smallest selected one the lowest indices."""
    idx, val = got.indices["model"].long(), got["model"]
    assert idx.numel() == val.numel() == k and bool((idx[1:] > idx[:-1]).all()) and 0 <= int(idx[0]) and int(idx[-1]) < x.numel()
    assert torch.equal(val.view(torch.int32), x[idx].view(torch.int32))
    key = x.view(torch.int32) & 0x7FFFFFFF
    t = int(key[idx].min())
    sel = torch.zeros(x.numel(), dtype=torch.bool, device=x.device)
    sel[idx] = True
    assert int(key[~sel].max()) <= t
    ties = (key == t).nonzero().flatten()
    taken = int(sel[ties].sum())
    assert bool(sel[ties[:taken]].all())


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _line(res, name, ts, **extra):
    res[name] = {"ms": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), **extra}
    print(f"{name:16s} {res[name]['ms']:10.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})  "
          + "  ".join(f"{k} {v}" for k, v in extra.items()), flush=True)


def run(P, rounds):
    import cloudpickle
    from flame_amd import egress, engine, sparse
    dev = torch.device("cuda", 0)
    w = torch.empty(P, dtype=torch.float32, device=dev)
    step = torch.empty(P, dtype=torch.float32, device=dev)
    engine.synth_fill_(w, 7, 0, 0, 1.0)
    engine.synth_fill_(step, 7, 1, 0, 0.01)
    dst = torch.empty_like(w)
    msg = {"weights": {"model": w}, "round": 1}
    arms = [("copy", lambda: dst.copy_(w), _events)]
    kernel = {r: [] for r in RATIOS}            # the call's own events (engine.kernel_events): the kernels without the launcher

    def native(ratio):
        engine.kernel_events = []
        out = engine.topk({"model": w}, ratio)
        evs, engine.kernel_events = engine.kernel_events, None
        assert len(evs) == 1 and evs[0][0] == "flame_topk_select", evs
        kernel[ratio].append(evs[0])
        return out
    for r in RATIOS:
        arms.append((f"native/{r}", lambda r=r: native(r), _events))
        arms.append((f"torch/{r}", lambda r=r: sparse.topk({"model": w}, r), _events))
    encoders = {"plain": egress.MessageEncoder(), "e2m1": egress.MessageEncoder(mx="e2m1"),
                "sparse": egress.MessageEncoder(sparse=0.01)}
    for nm, enc in encoders.items():
        arms.append((f"encode/{nm}", lambda e=enc: len(e.encode(msg)), _host))
    # every arm's output under the contract, before any time counts
    for r in RATIOS:
        k = math.ceil(r * P)
        _check(engine.topk({"model": w}, r), w, k)
        _check(sparse.topk({"model": w}, r).to(dev), w, k)
    trainer = {}
    for _ in range(3):                          # dense, then two sparse messages: the trainer holds the encoder's base
        got = cloudpickle.loads(bytes(encoders["sparse"].encode(msg)))["weights"]
        sparse.apply_(trainer, got)
        assert torch.equal(trainer["model"].view(torch.int32), encoders["sparse"]._base["model"].cpu().view(torch.int32))
        w.add_(step)
    assert isinstance(got, sparse.SparseWeights) and got["model"].numel() == math.ceil(0.01 * P)
    del trainer, got
    times, sizes = {nm: [] for nm, _, _ in arms}, {}
    for r in range(rounds + 1):                 # round 0 warms up
        for nm, fn, clock in (arms if r % 2 == 0 else arms[::-1]):
            if nm == "encode/sparse":
                w.add_(step)                    # the model moves between two messages
            torch.cuda.synchronize()
            ms, out = clock(fn)
            torch.cuda.synchronize()
            if nm.startswith("encode/"):
                sizes[nm] = out
            del out
            if r:
                times[nm].append(ms)
    res = {}
    copy_ms = statistics.median(times["copy"])
    copy_gbps = 8 * P / copy_ms / 1e6
    _line(res, "copy", times["copy"], GBps=round(copy_gbps, 1))
    five = 5 * 4 * P                            # the bytes of five reads of the source
    for r in RATIOS:
        n_ms, t_ms = statistics.median(times[f"native/{r}"]), statistics.median(times[f"torch/{r}"])
        k_ms = statistics.median(e0.elapsed_time(e1) for _, e0, e1, _ in kernel[r][-rounds:])
        _line(res, f"native/{r}", times[f"native/{r}"], kernels_ms=round(k_ms, 4), five_reads_GBps=round(five / k_ms / 1e6, 1),
              copy_probe_ms=round(five / copy_gbps / 1e6, 4), kernels_x_probe=round(k_ms / (five / copy_gbps / 1e6), 3))
        _line(res, f"torch/{r}", times[f"torch/{r}"], x_native=round(t_ms / n_ms, 2))
    plain_ms = statistics.median(times["encode/plain"])
    for nm in encoders:
        ms = statistics.median(times[f"encode/{nm}"])
        _line(res, f"encode/{nm}", times[f"encode/{nm}"], payload_bytes=sizes[f"encode/{nm}"],
              bytes_ratio=round(sizes[f"encode/{nm}"] / sizes["encode/plain"], 4), time_ratio=round(ms / plain_ms, 4))
    print(json.dumps({"metric": "topk_rate", "params": P, "rounds": rounds, "arms": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=25_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    torch.empty(1, device="cuda:0")
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)
    run(a.params, a.rounds)


if __name__ == "__main__":
    main()
