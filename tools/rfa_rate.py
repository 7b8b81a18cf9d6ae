#!/usr/bin/env python3
"""What the geometric median (RFA, ``FedAvg(rfa=T)``) costs, in ONE process on ONE device-resident
slab: after the bench's HBM settling, round by round and in alternating order,

  kernels (HIP-event kernel times, engine.kernel_events, recorded on the launch stream)
    FedAvg           engine.accumulate    -> flame_agg_reduce    (reads the slab once, writes the model)
    update guard     engine.update_stats  -> flame_update_stats  (reads the slab once: the yardstick)
    RFA's measure    engine.update_dist   -> flame_update_dist   (the same pass + one centre)
  whole rounds (HIP events on the current stream around ``do()``: kernels, host arithmetic and the
  readbacks between them)
    FedAvg(rfa=T).do for T in 1, 3, 5    -- 2T passes over the slab by count
    FedAvg(krum=n // 4).do               -- the Gram matrix + one reduction, for choosing between them

over the same N tiled slots of one UpdateSlab; medians over the rounds, the kernels' ratio to
flame_update_stats, the rounds' ratio to 2T plain reductions and to the Krum round.

    python tools/rfa_rate.py                                  # 64 x 25M fp32
    python tools/rfa_rate.py --clients 1024 --params 2000000
"""
import argparse
import collections
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TR = collections.namedtuple("TR", "weights count version")


class Cache(collections.OrderedDict):
    """The two calls an optimizer makes on flame's cache."""

    def iterkeys(self):
        return iter(list(self.keys()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--params", type=int, default=25_000_000)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16", "f64"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-settle", action="store_true")
    ap.add_argument("--no-krum", action="store_true")
    a = ap.parse_args()
    from flame_amd import engine
    from flame_amd.optimizer import FedAvg
    from flame_amd.slab import UpdateSlab
    dev = torch.device("cuda", 0)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}[a.dtype]
    n, P = a.clients, a.params
    slab = UpdateSlab({"model": torch.empty(P, dtype=dt)}, capacity=n, device=dev)
    fill = torch.empty(P, dtype=torch.float32 if dt == torch.float64 else dt, device=dev)
    slots = []
    for i in range(n):
        engine.synth_fill_(fill, 7, 1 + i, 0, 1e-2)
        slots.append(slab.put({"model": fill.to(dt)}))
    engine.synth_fill_(fill, 7, 0, 0, 1.0)
    agg = {"model": fill.to(dt).clone()}
    engine.synth_fill_(fill, 7, n + 1, 0, 1e-2)
    centre = {"model": fill.to(dt).clone()}
    del fill
    torch.cuda.synchronize()
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)
    entries = [(w, 1.0 / n) for w in slots]
    kernels = [("reduce", "flame_agg_reduce", lambda: engine.accumulate(agg, entries)),
               ("stats", "flame_update_stats", lambda: engine.update_stats(slots, dev)),
               ("dist", "flame_update_dist", lambda: engine.update_dist(slots, centre, dev))]

    def round_of(opt):
        def run():
            cache = Cache((f"e{i:05d}", TR(w, 1, 0)) for i, w in enumerate(slots))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.do(agg, cache, total=n)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run
    rounds = [(f"rfa{T}", round_of(FedAvg(rfa=T))) for T in (1, 3, 5)]
    if not a.no_krum and n <= engine.gram_max_clients() and n >= 2 * (n // 4) + 3:
        rounds.append(("krum", round_of(FedAvg(krum=n // 4))))
    arms = [(nm, kernel, fn) for nm, kernel, fn in kernels] + [(nm, None, fn) for nm, fn in rounds]
    times = {nm: [] for nm, _, _ in arms}
    read_bytes = n * P * agg["model"].element_size()
    for r in range(a.rounds + 1):               # round 0 warms up
        for nm, kernel, fn in (arms if r % 2 == 0 else arms[::-1]):
            if kernel is None:
                ms = fn()
            else:
                engine.kernel_events = []
                fn()
                torch.cuda.synchronize()
                evs, engine.kernel_events = engine.kernel_events, None
                assert len(evs) == 1 and evs[0][0] == kernel, evs
                ms = evs[0][1].elapsed_time(evs[0][2])
            if r:
                times[nm].append(ms)
    med = {nm: statistics.median(ts) for nm, ts in times.items()}
    res = {"metric": "rfa_rate", "clients": n, "params": P, "dtype": a.dtype, "rounds": a.rounds}
    for nm, kernel, _ in arms:
        ms = med[nm]
        res[nm] = {"ms_median": round(ms, 4), "ms_min": round(min(times[nm]), 4), "ms_max": round(max(times[nm]), 4)}
        if kernel is not None:
            res[nm].update(slab_GBps=round(read_bytes / ms / 1e6, 1), vs_stats=round(ms / med["stats"], 4))
            tail = f"{read_bytes / ms / 1e6:8.1f} GB/s of slab  x{ms / med['stats']:.4f} of flame_update_stats"
        elif nm.startswith("rfa"):
            T = int(nm[3:])
            res[nm].update(vs_2T_reduce=round(ms / (2 * T * med["reduce"]), 4))
            tail = f"x{ms / (2 * T * med['reduce']):.4f} of 2T = {2 * T} plain reductions"
            if "krum" in med:
                res[nm].update(vs_krum_round=round(ms / med["krum"], 4))
                tail += f"  x{ms / med['krum']:.4f} of the Krum round"
        else:
            tail = f"x{ms / med['reduce']:.4f} of one plain reduction"
        print(f"{nm:7s} {ms:9.4f} ms  (min {min(times[nm]):.4f}, max {max(times[nm]):.4f})  {tail}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
