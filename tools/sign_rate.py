#!/usr/bin/env python3
"""What a 1-bit sign uplink into an fp32 model costs, in ONE process (the shapes one after the other): after the
bench's HBM settling, round by round and in alternating order, one engine.accumulate over

  F32    fp32 updates                                          -> flame_agg_reduce
  E2M1   MXFP4 e2m1 updates, two per byte (mx.quantize)        -> flame_agg_reduce_mxfp4
  SIGN   sign bits + one fp32 scale per 256 (sign.compress)    -> flame_agg_reduce_sign

each as separate per-client tensors, once device-resident (``dev``) and once in pinned host memory (``host``: the
kernel reads the updates over the link, zero-copy -- the whole round from host memory).  Every arm is one kernel
(engine.kernel_events): its HIP-event time, and beside it the host's time to plan and issue the call
(``issue``: perf_counter around engine.accumulate, before any synchronise).  Medians over the rounds with min and
max, the bytes each arm moves (fp32: P (4n + 8); MXFP4: n ceil(P / 2) + n ceil(P / 32) + 8 P; sign:
8 n ceil(P / 64) + 4 n ceil(P / 256) + 8 P), GB/s, and for every arm its time and its bytes relative to the fp32
arm of the same residency: ``of the byte ratio`` is how far the arm is from its byte ratio (1.0 = exactly as
many times faster as it moves fewer bytes).  The sign arm's bits are checked once per shape and residency against
the fp32 round over sign.dequantize(update).  Everything printed also goes to ``--log``.

    python tools/sign_rate.py                              # the two shapes of DESIGN.md §4 -> profiles/sign_rate.log
    python tools/sign_rate.py --shape 64x25000000 --no-host
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

SHAPES = ("64x25000000", "1024x2000000")
ARMS = (("F32", "flame_agg_reduce"), ("E2M1", "flame_agg_reduce_mxfp4"), ("SIGN", "flame_agg_reduce_sign"))
_LOG = None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if _LOG is not None:
        _LOG.write(line + "\n")
        _LOG.flush()


def _bytes(arm, n, P):
    if arm == "F32":
        return P * (4 * n + 8)
    if arm == "E2M1":
        return n * -(-P // 2) + n * -(-P // 32) + 8 * P
    return 8 * n * -(-P // 64) + 4 * n * -(-P // 256) + 8 * P


def _updates(engine, mx, sign, n, P, dev, host):
    """{arm: [update per client]} on the device, and (``host``) the same bytes in pinned memory."""
    fill = torch.empty(P, dtype=torch.float32, device=dev)
    ups = {arm: [] for arm, _ in ARMS}
    for i in range(n):
        engine.synth_fill_(fill, 7, 1 + i, 0, 1e-2)
        ups["F32"].append({"model": fill.clone()})
        ups["E2M1"].append(mx.quantize({"model": fill}, "e2m1"))
        ups["SIGN"].append(sign.compress({"model": fill}))
    torch.cuda.synchronize()
    if not host:
        return ups, None

    def pin(t):
        if t.dtype == mx.PACKED:        # (a packed key is copied as its bytes)
            return pin(t.view(torch.uint8)).view(mx.PACKED)
        return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t)
    pinned = {"F32": [{"model": pin(u["model"])} for u in ups["F32"]],
              "E2M1": [mx.MXWeights({"model": pin(u["model"])}, {"model": pin(u.scales["model"])}, shapes=u.shapes) for u in ups["E2M1"]],
              "SIGN": [sign.SignWeights({"model": pin(u["model"])}, {"model": pin(u.scales["model"])}, u.shapes) for u in ups["SIGN"]]}
    torch.cuda.synchronize()
    return ups, pinned


def run(n, P, rounds, host):
    from flame_amd import engine, mx, sign
    dev = torch.device("cuda", 0)
    ups, pinned = _updates(engine, mx, sign, n, P, dev, host)
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
    times, issue = {nm: [] for nm, _, _, _ in arms}, {nm: [] for nm, _, _, _ in arms}
    for r in range(rounds + 1):                 # round 0 warms up
        for nm, kernel, fn, _ in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            engine.kernel_events = []
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            evs, engine.kernel_events = engine.kernel_events, None
            assert len(evs) == 1 and evs[0][0] == kernel, evs
            if r:
                times[nm].append(evs[0][1].elapsed_time(evs[0][2]))
                issue[nm].append((t1 - t0) * 1e3)
    # the sign rounds against the fp32 kernel over the dequantized updates, client by client: the same bits
    want = {"model": base.clone()}
    for u in ups["SIGN"]:
        engine.accumulate(want, [({"model": sign.dequantize(u)["model"]}, 1.0 / n)])
    for where, src in (("dev", ups), ("host", pinned)):
        if src is not None:
            got = {"model": base.clone()}
            engine.accumulate(got, [(w, 1.0 / n) for w in src["SIGN"]])
            assert torch.equal(got["model"].view(torch.int32), want["model"].view(torch.int32)), where
    aggs = {nm: agg for nm, _, _, agg in arms}
    if host:    # the same bytes read from either memory give the same bits
        assert all(torch.equal(aggs[f"{arm}/dev"]["model"].view(torch.int32), aggs[f"{arm}/host"]["model"].view(torch.int32)) for arm, _ in ARMS)
    res = {"metric": "sign_rate", "clients": n, "params": P, "rounds": rounds, "arms": {}}
    for nm in times:
        arm, where = nm.split("/")
        med, ref = statistics.median(times[nm]), statistics.median(times[f"F32/{where}"])
        b, b32 = _bytes(arm, n, P), _bytes("F32", n, P)
        t_ratio, b_ratio = med / ref, b / b32
        res["arms"][nm] = {"ms": round(med, 4), "min": round(min(times[nm]), 4), "max": round(max(times[nm]), 4),
                           "issue_ms": round(statistics.median(issue[nm]), 3), "bytes": b, "GBps": round(b / med / 1e6, 1),
                           "ms/F32": round(t_ratio, 4), "bytes/F32": round(b_ratio, 4), "x bytes": round(t_ratio / b_ratio, 3)}
        say(f"{n} x {P}  {nm:10s} {med:10.4f} ms  (min {min(times[nm]):.4f}, max {max(times[nm]):.4f}; issue "
            f"{statistics.median(issue[nm]):.3f} ms)  {b / 1e9:8.3f} GB  {b / med / 1e6:8.1f} GB/s  time x{t_ratio:.4f} of F32, "
            f"bytes x{b_ratio:.4f}, {t_ratio / b_ratio:.3f} of the byte ratio")
    say(json.dumps(res))
    del ups, pinned, arms, aggs, want
    torch.cuda.empty_cache()


def main():
    global _LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="CLIENTSxPARAMS, e.g. 64x25000000 (repeatable)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="leave the pinned-host arms out")
    ap.add_argument("--no-settle", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "sign_rate.log"))
    a = ap.parse_args()
    torch.empty(1, device="cuda:0")
    _LOG = open(a.log, "w")
    say("# tools/sign_rate.py", " ".join(sys.argv[1:]))
    if not a.no_settle:
        import bench
        say("settle:", json.dumps(bench.settle_hbm(max_s=10.0)))
    for shape in a.shape or SHAPES:
        n, P = (int(x) for x in shape.split("x"))
        run(n, P, a.rounds, not a.no_host)


if __name__ == "__main__":
    main()
