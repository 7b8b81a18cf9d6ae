#!/usr/bin/env python3
"""What a 16-bit uplink into an fp32 model costs, in ONE process per shape on device-resident slabs:
after the bench's HBM settling, round by round and in alternating order, HIP-event times of

  S32   fp32 updates into the fp32 model                 engine.accumulate -> flame_agg_reduce
  S16   bf16 / f16 updates into a model of that dtype    engine.accumulate -> flame_agg_reduce
  M16   bf16 / f16 updates into the fp32 model           engine.accumulate -> flame_agg_reduce_mixed
  P16   M16's inputs through engine._accumulate_promoted (per client one temporary in the update's
        dtype and one in fp32, then a rate-1 reduction: the route before flame_agg_reduce_mixed)

S32 / S16 / M16 are one kernel each (engine.kernel_events); P16 is 2n + 1 launches, timed by events
around the call on the launch stream, with the peak of its temporaries.  Medians over the rounds;
by bytes M16 / S16 should be (2n + 8) / (2n + 4) and M16 / S32 (2n + 8) / (4n + 8).

``--ingest``: 64 x 25M pinned host updates through DeviceUpdateCache(placement="slab") and
FedAvg.do, bf16 against fp32, wall clock from the first insert to the synchronised result.

    python tools/uplink16_rate.py                       # the two shapes of DESIGN.md §4, bf16 and f16
    python tools/uplink16_rate.py --shape 64x25000000 --dtype bf16 --ingest
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = ("64x25000000", "1024x2000000")


def _slab(engine, n, P, dt, dev):
    from flame_amd.slab import UpdateSlab
    slab = UpdateSlab({"model": torch.empty(P, dtype=dt)}, capacity=n, device=dev)
    fill = torch.empty(P, dtype=dt, device=dev)
    slots = []
    for i in range(n):
        engine.synth_fill_(fill, 7, 1 + i, 0, 1e-2)
        slots.append(slab.put({"model": fill}))
    torch.cuda.synchronize()
    return slab, slots


def run(n, P, dtype, rounds, promoted):
    from flame_amd import engine
    dev = torch.device("cuda", 0)
    dt = DTYPES[dtype]
    slab32, slots32 = _slab(engine, n, P, torch.float32, dev)
    slab16, slots16 = _slab(engine, n, P, dt, dev)
    base = torch.empty(P, dtype=torch.float32, device=dev)
    engine.synth_fill_(base, 7, 0, 0, 1.0)
    agg32, agg16, aggm, aggp = {"model": base.clone()}, {"model": base.to(dt)}, {"model": base.clone()}, {"model": base.clone()}
    del base
    e32 = [(w, 1.0 / n) for w in slots32]
    e16 = [(w, 1.0 / n) for w in slots16]
    arms = [("S32", "flame_agg_reduce", lambda: engine.accumulate(agg32, e32)),
            ("S16", "flame_agg_reduce", lambda: engine.accumulate(agg16, e16)),
            ("M16", "flame_agg_reduce_mixed", lambda: engine.accumulate(aggm, e16))]
    if promoted:
        arms.append(("P16", None, lambda: engine._accumulate_promoted(aggp, "model", e16, dev)))
    times = {nm: [] for nm, _, _ in arms}
    peak = 0
    for r in range(rounds + 1):                 # round 0 warms up
        for nm, kernel, fn in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            if kernel is None:
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
                peak = max(peak, torch.cuda.max_memory_allocated(dev) - before)
            else:
                engine.kernel_events = []
                fn()
                torch.cuda.synchronize()
                evs, engine.kernel_events = engine.kernel_events, None
                assert len(evs) == 1 and evs[0][0] == kernel, evs
                ms = evs[0][1].elapsed_time(evs[0][2])
            if r:
                times[nm].append(ms)
    if promoted:        # the two routes agree bit for bit after the same number of rounds
        assert torch.equal(aggm["model"].view(torch.int32), aggp["model"].view(torch.int32))
    med = {nm: statistics.median(t) for nm, t in times.items()}
    byt = {"S32": P * (4 * n + 8), "S16": P * (2 * n + 4), "M16": P * (2 * n + 8)}
    res = {"metric": "uplink16_rate", "clients": n, "params": P, "dtype": dtype, "rounds": rounds,
           "ms": {nm: round(v, 4) for nm, v in med.items()},
           "ms_min_max": {nm: [round(min(t), 4), round(max(t), 4)] for nm, t in times.items()},
           "GBps": {nm: round(byt[nm] / med[nm] / 1e6, 1) for nm in byt},
           "M16/S16": round(med["M16"] / med["S16"], 4), "M16/S16 by bytes": round((2 * n + 8) / (2 * n + 4), 4),
           "M16/S32": round(med["M16"] / med["S32"], 4), "M16/S32 by bytes": round((2 * n + 8) / (4 * n + 8), 4)}
    if promoted:
        res["P16/M16"] = round(med["P16"] / med["M16"], 2)
        res["P16 temporaries GB"] = round(peak / 1e9, 3)
    for nm in med:
        print(f"{n} x {P} {dtype}  {nm}  {med[nm]:10.4f} ms  (min {min(times[nm]):.4f}, max {max(times[nm]):.4f})", flush=True)
    print(json.dumps(res), flush=True)
    del slots32, slots16, slab32, slab16, e32, e16, arms, agg32, agg16, aggm, aggp
    torch.cuda.empty_cache()


def ingest(n, P, rounds):
    """Pinned host updates -> DeviceUpdateCache -> FedAvg.do: bf16 against fp32 updates, fp32 model."""
    from flame_amd.ingest import DeviceUpdateCache
    from flame_amd.optimizers import optimizer_provider
    dev = torch.device("cuda", 0)

    class TR:
        def __init__(self, w, c):
            self.weights, self.count, self.version = w, c, 0

    g = torch.Generator().manual_seed(3)
    src = torch.randn(P, generator=g) * 1e-2
    host = {"f32": [src.clone().pin_memory() for _ in range(n)], "bf16": [src.to(torch.bfloat16).pin_memory() for _ in range(n)]}
    base = {"model": torch.randn(P, generator=g).to(dev)}
    opt = optimizer_provider.get("fedavg")
    times = {k: [] for k in host}
    for r in range(rounds + 1):
        for name in (list(host) if r % 2 == 0 else list(host)[::-1]):
            cache = DeviceUpdateCache(dev, placement="slab", capacity=n)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, h in enumerate(host[name]):
                cache[f"e{i:04d}"] = TR({"model": h}, 1)
            opt.do(base, cache, total=n)
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) * 1e3)
            del cache
            torch.cuda.empty_cache()
    res = {"metric": "uplink16_ingest", "clients": n, "params": P, "rounds": rounds,
           "ms": {k: round(statistics.median(v), 2) for k, v in times.items()}}
    res["bf16/f32"] = round(res["ms"]["bf16"] / res["ms"]["f32"], 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="CLIENTSxPARAMS, e.g. 64x25000000 (repeatable)")
    ap.add_argument("--dtype", action="append", choices=list(DTYPES), help="the 16-bit dtype (repeatable; default both)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-promoted", action="store_true", help="leave the P16 arm out")
    ap.add_argument("--ingest", action="store_true", help="also the host ingest arm (64 x 25M)")
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    torch.empty(1, device="cuda:0")
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)
    for shape in a.shape or SHAPES:
        n, P = (int(x) for x in shape.split("x"))
        for dtype in a.dtype or list(DTYPES):
            run(n, P, dtype, a.rounds, not a.no_promoted)
    if a.ingest:
        ingest(64, 25_000_000, 3)


if __name__ == "__main__":
    main()
