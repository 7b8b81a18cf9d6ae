#!/usr/bin/env python3
"""What an MXFP8 or MXFP4 uplink into an fp32 model costs, in ONE process (the shapes one after the other): after
the bench's HBM settling, round by round and in alternating order, HIP-event times of one engine.accumulate over

  F32    fp32 updates                       -> flame_agg_reduce
  BF16   bf16 updates                       -> flame_agg_reduce_mixed
  E4M3   MXFP8 e4m3 updates (mx.quantize)   -> flame_agg_reduce_mx
  E5M2   MXFP8 e5m2 updates                 -> flame_agg_reduce_mx
  E2M1   MXFP4 e2m1 updates, two per byte   -> flame_agg_reduce_mxfp4

each as separate per-client tensors, once device-resident (``dev``) and once in pinned host memory
(``host``: the kernel reads the updates over the link, zero-copy -- the whole round from host memory).
Every arm is one kernel (engine.kernel_events).  Medians over the rounds, the bytes each arm moves
(fp32: P (4n + 8); bf16: P (2n + 8); MXFP8: P (n + 8) + n ceil(P / 32); MXFP4: n ceil(P / 2) + 8 P +
n ceil(P / 32)), GB/s, and for every arm its time
and its bytes relative to the fp32 arm of the same residency: ``x bytes`` is how far the arm is from
its byte ratio (1.0 = exactly as many times faster as it moves fewer bytes).

    python tools/mx_rate.py                             # the two shapes of DESIGN.md §4
    python tools/mx_rate.py --shape 64x25000000 --no-host
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("64x25000000", "1024x2000000")
ARMS = (("F32", "flame_agg_reduce"), ("BF16", "flame_agg_reduce_mixed"), ("E4M3", "flame_agg_reduce_mx"),
        ("E5M2", "flame_agg_reduce_mx"), ("E2M1", "flame_agg_reduce_mxfp4"))


def _bytes(arm, n, P):
    if arm == "F32":
        return P * (4 * n + 8)
    if arm == "BF16":
        return P * (2 * n + 8)
    if arm == "E2M1":
        return n * -(-P // 2) + 8 * P + n * -(-P // 32)
    return P * (n + 8) + n * -(-P // 32)


def _updates(engine, mx, n, P, dev, host):
    """{arm: [update dict per client]} on the device, and (``host``) the same bytes in pinned memory."""
    fill = torch.empty(P, dtype=torch.float32, device=dev)
    ups = {arm: [] for arm, _ in ARMS}
    for i in range(n):
        engine.synth_fill_(fill, 7, 1 + i, 0, 1e-2)
        ups["F32"].append({"model": fill.clone()})
        ups["BF16"].append({"model": fill.to(torch.bfloat16)})
        ups["E4M3"].append(mx.quantize({"model": fill}, "e4m3"))
        ups["E5M2"].append(mx.quantize({"model": fill}, "e5m2"))
        ups["E2M1"].append(mx.quantize({"model": fill}, "e2m1"))
    torch.cuda.synchronize()
    pinned = None
    if host:
        def pin(t):
            if t.dtype == mx.PACKED:        # (a packed key is copied as its bytes)
                return pin(t.view(torch.uint8)).view(mx.PACKED)
            return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t)
        pinned = {arm: [mx.MXWeights({"model": pin(u["model"])}, {"model": pin(u.scales["model"])}, shapes=u.shapes)
                        if arm[0] == "E"
                        else {"model": pin(u["model"])} for u in us] for arm, us in ups.items()}
        torch.cuda.synchronize()
    return ups, pinned


def run(n, P, rounds, host):
    from flame_amd import engine, mx
    dev = torch.device("cuda", 0)
    ups, pinned = _updates(engine, mx, n, P, dev, host)
    base = torch.empty(P, dtype=torch.float32, device=dev)
    engine.synth_fill_(base, 7, 0, 0, 1.0)
    arms = []
    for where, src in (("dev", ups), ("host", pinned)):
        if src is None:
            continue
        for arm, kernel in ARMS:
            agg = {"model": base.clone()}
            entries = [(w, 1.0 / n) for w in src[arm]]
            arms.append((f"{arm}/{where}", kernel, (lambda a=agg, e=entries: engine.accumulate(a, e)), agg))
    times = {nm: [] for nm, _, _, _ in arms}
    for r in range(rounds + 1):                 # round 0 warms up
        for nm, kernel, fn, _ in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            engine.kernel_events = []
            fn()
            torch.cuda.synchronize()
            evs, engine.kernel_events = engine.kernel_events, None
            assert len(evs) == 1 and evs[0][0] == kernel, evs
            if r:
                times[nm].append(evs[0][1].elapsed_time(evs[0][2]))
    # the same bytes read from either memory give the same bits
    aggs = {nm: agg for nm, _, _, agg in arms}
    for arm, _ in ARMS:
        if host:
            assert torch.equal(aggs[f"{arm}/dev"]["model"].view(torch.int32), aggs[f"{arm}/host"]["model"].view(torch.int32)), arm
    med = {nm: statistics.median(t) for nm, t in times.items()}
    res = {"metric": "mx_rate", "clients": n, "params": P, "rounds": rounds, "arms": {}}
    for nm in med:
        arm, where = nm.split("/")
        b, b32 = _bytes(arm, n, P), _bytes("F32", n, P)
        t_ratio, b_ratio = med[nm] / med[f"F32/{where}"], b / b32
        res["arms"][nm] = {"ms": round(med[nm], 4), "min": round(min(times[nm]), 4), "max": round(max(times[nm]), 4),
                           "bytes": b, "GBps": round(b / med[nm] / 1e6, 1), "ms/F32": round(t_ratio, 4),
                           "bytes/F32": round(b_ratio, 4), "x bytes": round(t_ratio / b_ratio, 3)}
        print(f"{n} x {P}  {nm:10s} {med[nm]:10.4f} ms  (min {min(times[nm]):.4f}, max {max(times[nm]):.4f})  "
              f"{b / 1e9:8.3f} GB  {b / med[nm] / 1e6:8.1f} GB/s  time x{t_ratio:.3f} of F32, bytes x{b_ratio:.3f}, "
              f"{t_ratio / b_ratio:.3f} of the byte ratio", flush=True)
    print(json.dumps(res), flush=True)
    del ups, pinned, arms, aggs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="CLIENTSxPARAMS, e.g. 64x25000000 (repeatable)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="leave the pinned-host arms out")
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    torch.empty(1, device="cuda:0")
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)
    for shape in a.shape or SHAPES:
        n, P = (int(x) for x in shape.split("x"))
        run(n, P, a.rounds, not a.no_host)


if __name__ == "__main__":
    main()
