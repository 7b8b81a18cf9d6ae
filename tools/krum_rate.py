#!/usr/bin/env python3
"""What the pairwise Gram matrix (Krum / Multi-Krum's measuring pass) costs against the update
guard's statistics and the plain reduction, in ONE process on ONE device-resident slab: after the
bench's HBM settling, round by round and in alternating order, HIP-event kernel times
(engine.kernel_events, recorded on the launch stream) of

  FedAvg           engine.accumulate    -> flame_agg_reduce    (reads the slab once, writes the model)
  update guard     engine.update_stats  -> flame_update_stats  (reads the slab once: the yardstick)
  FedAvg(krum=f)   engine.update_gram   -> flame_update_gram   (fp64 matrix cores + its finish kernel)

over the same N tiled slots of one UpdateSlab; medians over the rounds, each one's ratio to
flame_update_stats, and for the Gram the fp64 rate over the upper 16-client blocks,
``n16 (n16 + 16) / 2 * 2 * P`` FLOP with n16 = N rounded up to 16.

    python tools/krum_rate.py                                  # 64 x 25M fp32
    python tools/krum_rate.py --clients 1024 --params 2000000
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--params", type=int, default=25_000_000)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16", "f64"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    from flame_amd import engine
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
    del fill
    torch.cuda.synchronize()
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)
    entries = [(w, 1.0 / n) for w in slots]
    arms = [("reduce", "flame_agg_reduce", lambda: engine.accumulate(agg, entries)),
            ("stats", "flame_update_stats", lambda: engine.update_stats(slots, dev)),
            ("gram", "flame_update_gram", lambda: engine.update_gram(slots, dev))]
    times = {nm: [] for nm, _, _ in arms}
    read_bytes = n * P * agg["model"].element_size()
    for r in range(a.rounds + 1):               # round 0 warms up
        for nm, kernel, fn in (arms if r % 2 == 0 else arms[::-1]):
            engine.kernel_events = []
            fn()
            torch.cuda.synchronize()
            evs, engine.kernel_events = engine.kernel_events, None
            assert len(evs) == 1 and evs[0][0] == kernel, evs
            if r:
                times[nm].append(evs[0][1].elapsed_time(evs[0][2]))
    ref_ms = statistics.median(times["stats"])
    n16 = -(-n // 16) * 16
    flop = n16 * (n16 + 16) // 2 * 2 * P
    res = {"metric": "krum_rate", "clients": n, "params": P, "dtype": a.dtype, "rounds": a.rounds, "gram_flop": flop}
    for nm, _, _ in arms:
        ms = statistics.median(times[nm])
        res[nm] = {"ms_median": round(ms, 4), "ms_min": round(min(times[nm]), 4), "ms_max": round(max(times[nm]), 4),
                   "slab_GBps": round(read_bytes / ms / 1e6, 1), "vs_stats": round(ms / ref_ms, 4)}
        extra = f"  {flop / ms / 1e9:7.2f} TFLOP/s fp64" if nm == "gram" else ""
        if nm == "gram":
            res[nm]["fp64_TFLOPs"] = round(flop / ms / 1e9, 2)
        print(f"{nm:7s} {ms:9.4f} ms  (min {min(times[nm]):.4f}, max {max(times[nm]):.4f})  "
              f"{read_bytes / ms / 1e6:8.1f} GB/s of slab  x{ms / ref_ms:.4f} of flame_update_stats{extra}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
