#!/usr/bin/env python3
"""What the MX downlink costs, in ONE process after the bench's HBM settling, the arms alternating.

Arm 1, the quantiser alone: ``engine.mx_quantize`` (one flame_mx_quantize launch) against ``mx.quantize`` (the
torch-op route a user has without it) on the same device tensor of ``--params`` fp32 parameters, per element
format; device events around each call, medians over ``--rounds`` rounds with min and max, and for the native arm
the launch's own events as well (the kernel without its launcher).  Beside the kernel's time stands the same
process's streaming-copy probe for its bytes (4 B read and 1 + 1/32 B, or 1/2 + 1/32 B, written per parameter):
the rate of ``dst.copy_(src)`` over an fp32 tensor of that size, read plus written bytes.

Arm 2, the message: ``MessageEncoder.encode`` of ``{"weights": {"model": w}, "round": r}`` plain, with
``mx="e4m3"`` and with ``mx="e2m1"``; ``encode`` ends in a synchronise, so a host clock around it is valid.

Every arm's output is compared with ``mx.quantize``'s under the contract before its time counts.

    python tools/mx_downlink_rate.py                    # 25M parameters: the README's 100 MB model
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

FMTS = ("e4m3", "e5m2", "e2m1")


def _check(got, ref, fmt):
    """``got`` against ``ref`` (both MXWeights on the device): scale bytes equal, element bytes equal where the
    reference is not a NaN, a NaN where it is one."""
    assert torch.equal(got.scales["model"], ref.scales["model"]), fmt
    g, r = got["model"].view(torch.uint8).reshape(-1), ref["model"].view(torch.uint8).reshape(-1)
    nan = (r & 0x7F) > {"e4m3": 0x7E, "e5m2": 0x7C, "e2m1": 0xFF}[fmt]
    assert bool(((g == r) | nan).all()) and bool(((g[nan] & 0x7F) > (0x7E if fmt == "e4m3" else 0x7C)).all()), fmt


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def _line(res, name, ts, **extra):
    res[name] = {"ms": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), **extra}
    print(f"{name:16s} {res[name]['ms']:10.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})  "
          + "  ".join(f"{k} {v}" for k, v in extra.items()), flush=True)


def run(P, rounds):
    import cloudpickle
    from flame_amd import egress, engine, mx
    dev = torch.device("cuda", 0)
    w = torch.empty(P, dtype=torch.float32, device=dev)
    engine.synth_fill_(w, 7, 0, 0, 1.0)
    dst = torch.empty_like(w)
    msg = {"weights": {"model": w}, "round": 1}
    arms = [("copy", lambda: dst.copy_(w), _events)]
    kernel = {fmt: [] for fmt in FMTS}          # the launch's own events (engine.kernel_events): the kernel without its launcher

    def native(fmt):
        engine.kernel_events = []
        out = engine.mx_quantize({"model": w}, fmt)
        evs, engine.kernel_events = engine.kernel_events, None
        assert len(evs) == 1 and evs[0][0] == "flame_mx_quantize", evs
        kernel[fmt].append(evs[0])
        return out
    for fmt in FMTS:
        arms.append((f"native/{fmt}", lambda f=fmt: native(f), _events))
        arms.append((f"torch/{fmt}", lambda f=fmt: mx.quantize({"model": w}, f), _events))
    encoders = {"plain": egress.MessageEncoder(), "e4m3": egress.MessageEncoder(mx="e4m3"),
                "e2m1": egress.MessageEncoder(mx="e2m1")}
    for nm, enc in encoders.items():
        arms.append((f"encode/{nm}", lambda e=enc: len(e.encode(msg)), _host))
    # every arm's output under the contract, before any time counts
    for fmt in FMTS:
        _check(engine.mx_quantize({"model": w}, fmt), mx.quantize({"model": w}, fmt), fmt)
    for nm in ("e4m3", "e2m1"):
        got = cloudpickle.loads(bytes(encoders[nm].encode(msg)))["weights"]
        _check(got.to(dev), mx.quantize({"model": w}, nm), nm)
    times, sizes = {nm: [] for nm, _, _ in arms}, {}
    for r in range(rounds + 1):                 # round 0 warms up
        for nm, fn, clock in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            ms, out = clock(fn)
            torch.cuda.synchronize()
            if nm.startswith("encode/"):
                sizes[nm] = out
            del out
            if r:
                times[nm].append(ms)
    res = {}
    copy_ms = statistics.median(times["copy"])
    copy_gbps = 8 * P / copy_ms / 1e6
    _line(res, "copy", times["copy"], GBps=round(copy_gbps, 1))
    for fmt in FMTS:
        b = 4 * P + engine.mx_out_bytes(fmt, P) + mx.n_blocks(P)
        n_ms, t_ms = statistics.median(times[f"native/{fmt}"]), statistics.median(times[f"torch/{fmt}"])
        k_ms = statistics.median(e0.elapsed_time(e1) for _, e0, e1, _ in kernel[fmt][-rounds:])
        _line(res, f"native/{fmt}", times[f"native/{fmt}"], kernel_ms=round(k_ms, 4), kernel_GBps=round(b / k_ms / 1e6, 1),
              copy_probe_ms=round(b / copy_gbps / 1e6, 4), kernel_x_probe=round(k_ms / (b / copy_gbps / 1e6), 3))
        _line(res, f"torch/{fmt}", times[f"torch/{fmt}"], x_native=round(t_ms / n_ms, 2))
    plain_ms = statistics.median(times["encode/plain"])
    for nm in encoders:
        ms = statistics.median(times[f"encode/{nm}"])
        _line(res, f"encode/{nm}", times[f"encode/{nm}"], payload_bytes=sizes[f"encode/{nm}"],
              bytes_ratio=round(sizes[f"encode/{nm}"] / sizes["encode/plain"], 4), time_ratio=round(ms / plain_ms, 4))
    print(json.dumps({"metric": "mx_downlink_rate", "params": P, "rounds": rounds, "arms": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=25_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    torch.empty(1, device="cuda:0")
    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)
    run(a.params, a.rounds)


if __name__ == "__main__":
    main()
