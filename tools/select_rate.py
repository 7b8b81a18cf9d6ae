#!/usr/bin/env python3
"""What the trimmed mean by radix selection costs against the plain reduction and against the chain
kernel, in ONE process on ONE device-resident slab per shape: after the bench's HBM settling, round
by round and in alternating order, HIP-event kernel times (engine.kernel_events, recorded on the
launch stream) of

  FedAvg                       engine.accumulate     -> flame_agg_reduce   (the yardstick)
  FedAvg(trim=k)               engine.trimmed_mean   -> flame_agg_trimmed  for k <= 16 (the chain)
  FedAvg(trim=k, "select")     engine.selected_mean  -> flame_agg_select   for every k

over the same N tiled slots of one UpdateSlab; medians over the rounds, each arm's ratio to the
plain reduction and the number of passes the selection makes over the slab (key bits / 4 digit
passes per group of elements searched, plus the summing pass).

    python tools/select_rate.py                       # the three shapes of DESIGN.md §4
    python tools/select_rate.py --shape 1024x2000000xf32 --k 102,511
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
SHAPES = (("64x25000000xf32", (2, 8, 16, 31)), ("64x25000000xbf16", (2, 8, 16, 31)), ("1024x2000000xf32", (102, 511)))
KERNEL = {"plain": "flame_agg_reduce", "chain": "flame_agg_trimmed", "select": "flame_agg_select"}


def passes(dtype: str) -> int:
    """Passes of the selection kernel over the slab: one per 4-bit digit of the key and group of
    elements searched side by side (bf16 / f16: two groups of four), and the summing pass."""
    bits, groups = {"f32": (32, 1), "bf16": (16, 2), "f16": (16, 2), "f64": (64, 1)}[dtype]
    return bits // 4 * groups + 1


def run(n, P, dtype, ks, rounds, max_chain):
    from flame_amd import engine
    from flame_amd.slab import UpdateSlab
    dev = torch.device("cuda", 0)
    dt = DTYPES[dtype]
    slab = UpdateSlab({"model": torch.empty(P, dtype=dt)}, capacity=n, device=dev)
    fill = torch.empty(P, dtype=torch.float32 if dt == torch.float64 else dt, device=dev)
    slots = []
    for i in range(n):
        engine.synth_fill_(fill, 7, 1 + i, 0, 1e-2)
        slots.append(slab.put({"model": fill.to(dt)}))
    engine.synth_fill_(fill, 7, 0, 0, 1.0)
    agg = {"model": fill.to(dt).clone()}
    del fill
    torch.cuda.synchronize()
    entries = [(w, 1.0 / n) for w in slots]
    arms = [("plain", "plain", lambda: engine.accumulate(agg, entries))]
    for k in ks:
        if k <= max_chain:
            arms.append((f"chain k={k}", "chain", (lambda k: lambda: engine.trimmed_mean(agg, slots, k))(k)))
        arms.append((f"select k={k}", "select", (lambda k: lambda: engine.selected_mean(agg, slots, k))(k)))
    times = {nm: [] for nm, _, _ in arms}
    read_bytes = n * P * agg["model"].element_size()
    for r in range(rounds + 1):                 # round 0 warms up
        for nm, kind, fn in (arms if r % 2 == 0 else arms[::-1]):
            engine.kernel_events = []
            fn()
            torch.cuda.synchronize()
            evs, engine.kernel_events = engine.kernel_events, None
            assert len(evs) == 1 and evs[0][0] == KERNEL[kind], evs
            if r:
                times[nm].append(evs[0][1].elapsed_time(evs[0][2]))
    ref_ms = statistics.median(times["plain"])
    res = {"metric": "select_rate", "clients": n, "params": P, "dtype": dtype, "rounds": rounds, "arms": {}}
    for nm, kind, _ in arms:
        ms = statistics.median(times[nm])
        p = passes(dtype) if kind == "select" else 1
        res["arms"][nm] = {"ms_median": round(ms, 4), "ms_min": round(min(times[nm]), 4), "ms_max": round(max(times[nm]), 4),
                           "vs_plain": round(ms / ref_ms, 3), "passes": p,
                           "slab_GBps": round(read_bytes * p / ms / 1e6, 1)}
        print(f"{n} x {P} {dtype}  {nm:14s} {ms:10.4f} ms  (min {min(times[nm]):.4f}, max {max(times[nm]):.4f})  "
              f"x{ms / ref_ms:.3f} of the plain reduction  {p} pass(es), {read_bytes * p / ms / 1e6:8.1f} GB/s of slab reads",
              flush=True)
    print(json.dumps(res), flush=True)
    del slots, slab, agg, entries, arms
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="CLIENTSxPARAMSxDTYPE, e.g. 64x25000000xbf16 (repeatable)")
    ap.add_argument("--k", help="comma-separated trim counts for the --shape arguments")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    from flame_amd import engine
    shapes = SHAPES
    if a.shape:
        if not a.k:
            ap.error("--shape needs --k")
        shapes = tuple((s, tuple(int(k) for k in a.k.split(","))) for s in a.shape)
    torch.empty(1, device="cuda:0")
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)
    for shape, ks in shapes:
        n, P, dtype = shape.split("x")
        n, P = int(n), int(P)
        run(n, P, dtype, [k for k in ks if n > 2 * k], a.rounds, engine.trimmed_max_k())


if __name__ == "__main__":
    main()
