#!/usr/bin/env python3
"""What a low-rank uplink into an fp32 model costs against the route it replaces, in ONE process (the shapes one
after the other): after the bench's HBM settling, round by round and in alternating order,

  LR      engine.accumulate over LowRankWeights          -> one flame_agg_reduce_lowrank
  DENSE   lowrank.densify per client (one matmul and one m x n fp32 temporary each), then engine.accumulate over
          the dense fp32 updates                          -> n matmuls + flame_agg_reduce

over one m x m fp32 key, every client at the same rank, factors device-resident.  Two times per arm, medians over
the rounds with min and max: ``call``, HIP events on the stream around the whole arm, and for LR ``kernel``, the
launch's own event time (engine.kernel_events), from which the achieved fp32 matrix rate 2 m n K / t (K = n r) and
the bytes per second of the kernel's algorithmic bytes (every factor once, the model read and written).  The two
arms' results are compared: the largest difference in units of gamma_{K+n+2} (|base| + sum rate |U| |V|).

    python tools/lowrank_rate.py                              # the four shapes of DESIGN.md §4
    python tools/lowrank_rate.py --shape 64x4096x16xbf16
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("64x4096x16xf32", "64x4096x16xbf16", "64x4096x4xf32", "1024x1024x8xf32")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def run(n, m, r, dt, rounds, out):
    from flame_amd import engine, lowrank
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)
    ups = [lowrank.LowRankWeights({"w": (torch.randn(m, r, generator=g, device=dev) * 1e-2).to(DT[dt])},
                                  {"w": torch.randn(r, m, generator=g, device=dev).to(DT[dt])}, {"w": (m, m)}) for _ in range(n)]
    base = torch.randn(m, m, generator=g, device=dev)
    rates = [1.0 / n] * n
    aggs = {"LR": {"w": base.clone()}, "DENSE": {"w": base.clone()}}

    def dense():
        engine.accumulate(aggs["DENSE"], [(lowrank.densify(u), rt) for u, rt in zip(ups, rates)])
    arms = [("LR", lambda: engine.accumulate(aggs["LR"], list(zip(ups, rates)))), ("DENSE", dense)]
    call, kern = {nm: [] for nm, _ in arms}, []
    for rd in range(rounds + 1):                # round 0 warms up
        for nm, fn in (arms if rd % 2 == 0 else arms[::-1]):
            aggs[nm]["w"].copy_(base)
            torch.cuda.synchronize()
            engine.kernel_events = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            evs, engine.kernel_events = engine.kernel_events, None
            assert [ev[0] for ev in evs] == (["flame_agg_reduce_lowrank"] if nm == "LR" else ["flame_agg_reduce"] * len(evs)), evs
            if rd:
                call[nm].append(e0.elapsed_time(e1))
                if nm == "LR":
                    kern.append((evs[0][1].elapsed_time(evs[0][2]), evs[0][3]))
    K = n * r
    mag = base.double().abs()
    for u in ups:
        mag += u["w"].double().abs() @ u.right["w"].double().abs() / n
    gam = (K + n + 2) * 2.0 ** -24 / (1 - (K + n + 2) * 2.0 ** -24)
    diff = float(((aggs["LR"]["w"].double() - aggs["DENSE"]["w"].double()).abs() / (gam * mag)).max())
    assert diff <= 2.0, diff
    med = {nm: statistics.median(t) for nm, t in call.items()}
    k_ms, k_bytes = statistics.median(t for t, _ in kern), kern[0][1]
    flop = 2.0 * m * m * K
    res = {"metric": "lowrank_rate", "clients": n, "m": m, "n": m, "rank": r, "factor_dtype": dt, "rounds": rounds, "K": K,
           "lr_call_ms": round(med["LR"], 4), "lr_min": round(min(call["LR"]), 4), "lr_max": round(max(call["LR"]), 4),
           "dense_call_ms": round(med["DENSE"], 4), "dense_min": round(min(call["DENSE"]), 4), "dense_max": round(max(call["DENSE"]), 4),
           "speedup": round(med["DENSE"] / med["LR"], 3), "kernel_ms": round(k_ms, 4), "tflops": round(flop / k_ms / 1e9, 2),
           "kernel_bytes": k_bytes, "gbps": round(k_bytes / k_ms / 1e6, 1), "dense_temp_bytes": 4 * m * m * n,
           "max_diff_in_bound_units": round(diff, 4)}
    lines = [f"{n} x {m}x{m} r={r} {dt}  LR    call {med['LR']:9.4f} ms (min {min(call['LR']):.4f}, max {max(call['LR']):.4f})  kernel {k_ms:.4f} ms  "
             f"{flop / 1e9:.1f} GFLOP -> {res['tflops']} TFLOP/s fp32 matrix, {k_bytes / 1e6:.1f} MB -> {res['gbps']} GB/s",
             f"{n} x {m}x{m} r={r} {dt}  DENSE call {med['DENSE']:9.4f} ms (min {min(call['DENSE']):.4f}, max {max(call['DENSE']):.4f})  "
             f"{n} matmuls, {4 * m * m * n / 1e9:.2f} GB of temporaries  -> LR is x{res['speedup']} faster; results differ by "
             f"{diff:.3f} of the bound", json.dumps(res)]
    for ln in lines:
        print(ln, flush=True)
        out.write(ln + "\n")
    out.flush()
    del ups, aggs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="CLIENTSxMxRANKxDTYPE, e.g. 64x4096x16xbf16 (repeatable)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-settle", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowrank_rate.log"))
    a = ap.parse_args()
    torch.empty(1, device="cuda:0")
    with open(a.out, "w") as out:
        if not a.no_settle:
            import bench
            ln = "settle: " + json.dumps(bench.settle_hbm(max_s=10.0))
            print(ln, flush=True)
            out.write(ln + "\n")
        for shape in a.shape or SHAPES:
            n, m, r, dt = shape.split("x")
            run(int(n), int(m), int(r), dt, a.rounds, out)


if __name__ == "__main__":
    main()
