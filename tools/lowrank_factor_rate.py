#!/usr/bin/env python3
"""What the low-rank factoriser and the low-rank downlink cost, in ONE process after the bench's HBM settling, the
arms alternating.

Per workload (one 4,096 x 4,096 key at r = 16 and at r = 4; 64 keys of 1,024 x 1,024 at r = 8), on the same device
tensors: ``engine.lowrank_factor`` (one flame_lowrank_factor call, five launches, and the base's advance) against the
two routes the tree had before it -- ``lowrank.compress`` of ``W - base`` (torch's SVD) and the same three steps as
torch ops (``(W - base) @ Q``, ``torch.linalg.qr``, ``U.T @ (W - base)``).  Device events around each call, medians over
``--rounds`` rounds with min and max, and for the native arm the entry point's own events as well (the five kernels
without the launcher; run the tool under ``rocprofv3 --kernel-trace --stats`` for the split by kernel).  Beside it
stands the same process's streaming-copy probe for the factoriser's floor, two reads of W and of base: the rate of
``dst.copy_(src)`` over an fp32 tensor of the workload's size, read plus written bytes.

Then the message: ``MessageEncoder.encode`` of the first workload's model plain and with ``lowrank=16`` (the weights
move between messages, outside the clock); ``encode`` ends in a synchronise, so a host clock around it is valid.

    python tools/lowrank_factor_rate.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from topk_rate import _events, _host, _line  # noqa: E402

WORKLOADS = (("4096x4096/r16", 1, 4096, 16), ("4096x4096/r4", 1, 4096, 4), ("64x1024x1024/r8", 64, 1024, 8))


def run(rounds):
    from flame_amd import egress, engine, lowrank
    dev = torch.device("cuda", 0)
    res = {}
    for name, n_keys, side, r in WORKLOADS:
        g = torch.Generator(device=dev).manual_seed(1)
        base = {f"k{i}": torch.randn(side, side, device=dev, generator=g) for i in range(n_keys)}
        # a change of decaying spectrum on top of noise, as a model's update is
        w = {k: b + (torch.randn(side, 64, device=dev, generator=g) * torch.logspace(0, -3, 64, device=dev))
             @ torch.randn(64, side, device=dev, generator=g) * 0.01 for k, b in base.items()}
        q = {k: torch.randn(side, r, device=dev, generator=g) for k in base}
        src, dst = torch.empty(n_keys * side * side, device=dev), torch.empty(n_keys * side * side, device=dev)
        kernel = []

        def native():
            engine.kernel_events = []
            out = engine.lowrank_factor(w, r, base={k: b.clone() for k, b in base.items()}, q=q)
            evs, engine.kernel_events = engine.kernel_events, None
            kernel.append([e for e in evs if e[0] == "flame_lowrank_factor"][0])
            return out

        def steps():
            out = {}
            for k in w:
                d = w[k] - base[k]
                u = torch.linalg.qr(d @ q[k]).Q
                out[k] = (u, u.T @ d)
            return out
        arms = [("copy", lambda: dst.copy_(src), _events), ("native", native, _events),
                ("torch-steps", steps, _events),
                ("torch-svd", lambda: lowrank.compress({k: w[k] - base[k] for k in w}, r), _events)]
        sent, _ = native()                              # the output under the contract before any time counts
        for k in list(w)[:2]:
            u, v, d = sent[k].double(), sent.right[k].double(), (w[k] - base[k]).double()
            assert float((u.T @ u - torch.eye(r, device=dev)).abs().max()) <= 4 * r * 2.0 ** -24
            assert float((v - u.T @ d).abs().max()) <= 2.0 ** -24 * (side + 2) * float((u.abs().T @ d.abs()).max()) * 1.01
        times = {nm: [] for nm, _, _ in arms}
        for rd in range(rounds + 1):                    # round 0 warms up
            for nm, fn, clock in (arms if rd % 2 == 0 else arms[::-1]):
                if nm == "torch-svd" and rd > 2:        # seconds per call: two timed rounds
                    continue
                torch.cuda.synchronize()
                ms, out = clock(fn)
                torch.cuda.synchronize()
                del out
                if rd:
                    times[nm].append(ms)
        out = res[name] = {}
        print(name, flush=True)
        copy_gbps = 8 * src.numel() / statistics.median(times["copy"]) / 1e6
        floor_ms = 16 * src.numel() / copy_gbps / 1e6     # two reads of W and of base at the copy probe's rate
        _line(out, "copy", times["copy"], GBps=round(copy_gbps, 1))
        k_ms = statistics.median(e0.elapsed_time(e1) for _, e0, e1, _ in kernel[-rounds:])
        n_ms = statistics.median(times["native"])
        _line(out, "native", times["native"], kernels_ms=round(k_ms, 4), floor_ms=round(floor_ms, 4), kernels_x_floor=round(k_ms / floor_ms, 2))
        for nm in ("torch-steps", "torch-svd"):
            _line(out, nm, times[nm], x_native=round(statistics.median(times[nm]) / n_ms, 2))
        if name == WORKLOADS[0][0]:
            encs = {"plain": egress.MessageEncoder(), "lowrank": egress.MessageEncoder(lowrank=16)}
            model, sizes, et = dict(w), {}, {nm: [] for nm in encs}
            for rd in range(rounds + 2):                # the dense message and one factorised one warm up
                for nm, enc in encs.items():
                    for k in model:
                        model[k] = model[k] + 0.001         # the model moves between two messages
                    ms, sizes[nm] = _host(lambda e=enc: len(e.encode({"weights": model, "round": rd})))
                    if rd > 1:
                        et[nm].append(ms)
            for nm in encs:
                _line(out, f"encode/{nm}", et[nm], payload_bytes=sizes[nm], bytes_ratio=round(sizes[nm] / sizes["plain"], 5),
                      time_ratio=round(statistics.median(et[nm]) / statistics.median(et["plain"]), 4))
    print(json.dumps({"metric": "lowrank_factor_rate", "rounds": rounds, "workloads": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    torch.empty(1, device="cuda:0")
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)
    run(a.rounds)


if __name__ == "__main__":
    main()
