#!/usr/bin/env python3
"""What the server-side update guard costs on a device-resident slab, in ONE process: after the
bench's HBM settling, round by round and in alternating order, HIP-event times of

  1. flame_agg_reduce          the plain reduction (the yardstick: same library, same slab)
  2. flame_update_stats        the per-update sums of squares and non-finite counts
  3. flame_agg_reduce_scaled   the reduction with every clip scale < 1

over the same N tiled slots of one UpdateSlab.  The statistics read the same bytes as the
reduction and write almost nothing; they are held to the plain reduction's time + 10 %, the
scaled reduction to + 5 %.

    python tools/guard_overhead.py --clients 1024 --params 25000000 --dtype f32
    python tools/guard_overhead.py --clients 64 --params 25000000 --dtype bf16
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=1024)
    ap.add_argument("--params", type=int, default=25_000_000)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    from flame_amd import _native as N, engine
    from flame_amd.slab import UpdateSlab
    L = N.lib()
    dev = torch.device("cuda", 0)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    code = engine.dtype_code(dt)
    n, P = a.clients, a.params
    slab = UpdateSlab({"model": torch.empty(P, dtype=dt)}, capacity=n, device=dev)
    tmp = torch.empty(P, dtype=dt, device=dev)
    slots = []
    for i in range(n):
        engine.synth_fill_(tmp, 7, 1 + i, 0, 1e-2)
        slots.append(slab.put({"model": tmp}))
    engine.synth_fill_(tmp, 7, 0, 0, 1.0)
    model0 = tmp
    torch.cuda.synchronize()
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)

    rows = engine.slab_rows(slots, ["model"], {"model": P}, {"model": dt}, dev)
    ptrs, tile_bytes = rows["model"]
    out = torch.empty(P, dtype=dt, device=dev)
    seg = engine.Seg(P, out=out.data_ptr(), inp=model0.data_ptr(), clients=ptrs, tile_stride=tile_bytes)
    rates = [1.0 / n] * n
    scales = [0.25 + 0.5 * (i % 7) / 7 for i in range(n)]           # every one < 1
    p = engine.plan(code, [seg], rates, scales=scales)
    dm = torch.from_numpy(p.meta).to(dev)
    base = dm.data_ptr()
    segp, clp, r32p, r64p = base, base + p.off_clients, base + p.off_r32, base + p.off_r64
    sbytes = int(L.flame_update_stats_scratch_bytes(p.n_chunks, n))
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
    stats = torch.zeros(2 * n, dtype=torch.int64, device=dev)
    st = engine._stream_ptr(dev)
    read_bytes = n * P * out.element_size()
    print(f"scratch {sbytes} B = {100.0 * sbytes / read_bytes:.4f} % of the {read_bytes} B read", flush=True)

    def plain():
        N.check(L.flame_agg_reduce(code, 0, segp, 1, p.n_chunks, clp, n, r32p, r64p, st))

    def stat():
        N.check(L.flame_update_stats(code, segp, 1, p.n_chunks, clp, n, stats.data_ptr(), stats.data_ptr() + 8 * n,
                                     scratch.data_ptr(), sbytes, st))

    def scaled():
        N.check(L.flame_agg_reduce_scaled(code, 0, segp, 1, p.n_chunks, clp, n, r32p, r64p, base + p.off_s32,
                                          base + p.off_s64, st))

    arms = [("flame_agg_reduce", plain), ("flame_update_stats", stat), ("flame_agg_reduce_scaled", scaled)]
    times = {nm: [] for nm, _ in arms}
    for r in range(a.rounds + 1):               # round 0 warms up
        for nm, fn in (arms if r % 2 == 0 else arms[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r:
                times[nm].append(e0.elapsed_time(e1))
    # the statistics of the last launch against torch on a few clients (sanity, not a test)
    stats.zero_()
    stat()
    torch.cuda.synchronize()
    host = stats.cpu().numpy()
    sq = host[:n].view(np.float64)
    for i in (0, n - 1):
        ref = float(slab.read(slots[i].slot, "model").double().square().sum())
        assert abs(sq[i] - ref) <= 1e-9 * ref and host[n + i] == 0, (i, sq[i], ref)
    ref_ms = statistics.median(times["flame_agg_reduce"])
    res = {"metric": "guard_overhead", "clients": n, "params": P, "dtype": a.dtype, "rounds": a.rounds,
           "scratch_bytes": sbytes, "scratch_pct_of_read": 100.0 * sbytes / read_bytes}
    for nm, _ in arms:
        ms = statistics.median(times[nm])
        res[nm] = {"ms_median": round(ms, 4), "ms_min": round(min(times[nm]), 4), "ms_max": round(max(times[nm]), 4),
                   "read_GBps": round(read_bytes / ms / 1e6, 1), "vs_plain": round(ms / ref_ms, 4)}
        print(f"{nm:26s} {ms:9.4f} ms  (min {min(times[nm]):.4f}, max {max(times[nm]):.4f})  "
              f"{read_bytes / ms / 1e6:8.1f} GB/s read  x{ms / ref_ms:.4f} of the plain reduction", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
