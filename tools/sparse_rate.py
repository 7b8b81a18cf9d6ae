#!/usr/bin/env python3
"""What a top-k sparse uplink into an fp32 model costs, in ONE process (the shapes one after the other):
after the bench's HBM settling, round by round and in alternating order, one engine.accumulate over

  F32     fp32 updates                              -> flame_agg_reduce
  E2M1    MXFP4 e2m1 updates (mx.quantize)          -> flame_agg_reduce_mxfp4
  S0.1    sparse updates at density 0.1 %           -> flame_sparse_index + flame_agg_reduce_sparse
  S1      ... at 1 %
  S10     ... at 10 %

each as separate per-client tensors, once device-resident (``dev``) and once in pinned host memory
(``host``: the dense arms read the updates over the link zero-copy; the sparse arm copies values and
indices to the device once each, inside the timed call).  A sparse update keeps the elements with
``|x| > t`` for its own quantile ``t`` of ``|x|`` at its density, from one sort per update: what top-k keeps.
The achieved density of every arm is asserted to be within 0.1 % of its name.

Two times per arm, medians over the rounds with min and max: ``call``, HIP events on the stream around
the whole engine.accumulate (for the sparse arm that includes the copy of the validation counters, a
synchronisation point), and ``kernels``, the sum of the launches' own event times (engine.kernel_events);
for the sparse arm the index kernel's share of ``kernels``.  Bytes: fp32 P (4n + 8); MXFP4 n ceil(P / 2) +
8 P + n ceil(P / 32); sparse 8 nnz + 8 P (the bounds scratch is reported beside it).  ``x bytes`` is how far an
arm's call time is from its byte ratio to the fp32 arm of the same residency.

    python tools/sparse_rate.py                             # the two shapes of DESIGN.md §4
    python tools/sparse_rate.py --shape 64x25000000 --no-host
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("64x25000000", "1024x2000000")
DENSITY = {"S0.1": 0.001, "S1": 0.01, "S10": 0.1}
ARMS = ("F32", "E2M1", *DENSITY)
SIGMA = 1e-2


def _pin(t):
    return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t)


def _updates(engine, mx, sparse, n, P, dev, host):
    """{arm: [update per client]} on the device, and (``host``) the same bytes in pinned memory."""
    fill = torch.empty(P, dtype=torch.float32, device=dev)
    ups = {arm: [] for arm in ARMS}
    for i in range(n):
        engine.synth_fill_(fill, 7, 1 + i, 0, SIGMA)
        mags = fill.abs().sort().values     # the update's own quantiles of |x| (the generator is no normal: its tails end at 3.46 sigma)
        cut = {arm: mags[P - 1 - math.ceil(d * P)] for arm, d in DENSITY.items()}
        ups["F32"].append({"model": fill.clone()})
        ups["E2M1"].append(mx.quantize({"model": fill}, "e2m1"))
        for arm, t in cut.items():
            idx = (fill.abs() > t).nonzero().flatten()
            ups[arm].append(sparse.SparseWeights({"model": fill[idx]}, {"model": idx.to(torch.int32)}, {"model": (P,)}))
    torch.cuda.synchronize()
    for arm, d in DENSITY.items():      # every arm is at the density it is named for
        got = sum(u["model"].numel() for u in ups[arm]) / (n * P)
        assert abs(got / d - 1.0) < 0.001, (arm, got)
    pinned = None
    if host:
        pinned = {"F32": [{"model": _pin(u["model"])} for u in ups["F32"]],
                  "E2M1": [mx.MXWeights({"model": _pin(u["model"].view(torch.uint8)).view(mx.PACKED)},
                                        {"model": _pin(u.scales["model"])}, shapes=u.shapes) for u in ups["E2M1"]]}
        for arm in DENSITY:
            pinned[arm] = [sparse.SparseWeights({"model": _pin(u["model"])}, {"model": _pin(u.indices["model"])}, u.shapes)
                           for u in ups[arm]]
        torch.cuda.synchronize()
    return ups, pinned


def run(n, P, rounds, host):
    from flame_amd import engine, mx, sparse
    dev = torch.device("cuda", 0)
    ups, pinned = _updates(engine, mx, sparse, n, P, dev, host)
    base = torch.empty(P, dtype=torch.float32, device=dev)
    engine.synth_fill_(base, 7, 0, 0, 1.0)
    nnz = {arm: sum(u["model"].numel() for u in ups[arm]) for arm in DENSITY}
    nbytes = {"F32": P * (4 * n + 8), "E2M1": n * -(-P // 2) + 8 * P + n * -(-P // 32), **{a: 8 * nnz[a] + 8 * P for a in DENSITY}}
    arms = []
    for where, src in (("dev", ups), ("host", pinned)):
        if src is None:
            continue
        for arm in ARMS:
            agg = {"model": base.clone()}
            entries = [(w, 1.0 / n) for w in src[arm]]
            arms.append((f"{arm}/{where}", (lambda a=agg, e=entries: engine.accumulate(a, e)), agg))
    call, kern, share = ({nm: [] for nm, _, _ in arms} for _ in range(3))
    for r in range(rounds + 1):                 # round 0 warms up
        for nm, fn, _ in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            engine.kernel_events = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            evs, engine.kernel_events = engine.kernel_events, None
            assert len(evs) == (2 if nm[0] == "S" else 1), evs
            if r:
                ms = [ev[1].elapsed_time(ev[2]) for ev in evs]
                call[nm].append(e0.elapsed_time(e1))
                kern[nm].append(sum(ms))
                share[nm].append(ms[0] / sum(ms))
    aggs = {nm: agg for nm, _, agg in arms}
    for arm in ARMS:        # the same bytes read from either memory give the same bits
        if host:
            assert torch.equal(aggs[f"{arm}/dev"]["model"].view(torch.int32), aggs[f"{arm}/host"]["model"].view(torch.int32)), arm
    res = {"metric": "sparse_rate", "clients": n, "params": P, "rounds": rounds, "arms": {}}
    med = {nm: statistics.median(t) for nm, t in call.items()}
    for nm in med:
        arm, where = nm.split("/")
        t_ratio, b_ratio = med[nm] / med[f"F32/{where}"], nbytes[arm] / nbytes["F32"]
        row = {"call_ms": round(med[nm], 4), "min": round(min(call[nm]), 4), "max": round(max(call[nm]), 4),
               "kernels_ms": round(statistics.median(kern[nm]), 4), "bytes": nbytes[arm], "ms/F32": round(t_ratio, 4),
               "bytes/F32": round(b_ratio, 4), "x bytes": round(t_ratio / b_ratio, 3)}
        extra = ""
        if arm in DENSITY:
            row["nnz"], row["index_share"] = nnz[arm], round(statistics.median(share[nm]), 3)
            row["bounds_bytes"] = -(-P // 4096) * 4 * n * 8
            extra = (f"  nnz {nnz[arm]} ({100 * nnz[arm] / (n * P):.3f} %), index kernel {100 * row['index_share']:.0f} % of kernels, "
                     f"bounds {row['bounds_bytes'] / 1e6:.1f} MB")
        res["arms"][nm] = row
        print(f"{n} x {P}  {nm:10s} call {med[nm]:9.4f} ms (min {min(call[nm]):.4f}, max {max(call[nm]):.4f})  kernels "
              f"{row['kernels_ms']:9.4f} ms  {nbytes[arm] / 1e9:7.3f} GB  time x{t_ratio:.3f} of F32, bytes x{b_ratio:.3f}, "
              f"{t_ratio / b_ratio:.3f} of the byte ratio{extra}", flush=True)
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
