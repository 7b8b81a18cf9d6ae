#!/usr/bin/env python3
"""What the sign packer costs, in ONE process after the bench's HBM settling, the arms alternating.

Per shape (a 25M-element and a 2M-element fp32 model, each without and with a base) three arms on the same device
tensors: ``engine.sign_compress`` (one flame_onebit_pack launch); the same result as torch ops on the device
(``sign.compress`` of the model, or of ``model - base`` followed by ``base += dequantize``); and the streaming-copy
ceiling, ``dst.copy_(src)`` moving the launch's byte count (4 bytes per element without a base, 12 with one).  Device
events around each call, medians over ``--rounds`` rounds with min and max; for the native arm the call's own events
as well (the kernel without the launcher).  The native arm's output is checked bit for bit against
``sign.compress(fold=True)`` on the CPU before its time counts.  The lines go to stdout and to ``--log``.

    python tools/sign_pack_rate.py --log profiles/sign_pack_rate.log
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (25_000_000, 2_000_000)
_LOG = None


def _say(text):
    print(text, flush=True)
    if _LOG is not None:
        _LOG.write(text + "\n")
        _LOG.flush()


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _line(res, name, ts, **extra):
    res[name] = {"ms": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), **extra}
    _say(f"{name:18s} {res[name]['ms']:10.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})  " + "  ".join(f"{k} {v}" for k, v in extra.items()))


def _check(engine, sign, w, base):
    """One native call is ``sign.compress(fold=True)`` of ``w`` (of ``w - base``), and the base advanced by what was sent."""
    d = (w - base).cpu() if base is not None else w.cpu()
    b0 = base.cpu() if base is not None else None
    got = engine.sign_compress({"model": w}, base={"model": base} if base is not None else None)
    bits, scales = sign.compress_tensor(d, fold=True)
    assert torch.equal(got["model"].cpu(), bits) and torch.equal(got.scales["model"].cpu().view(torch.int32), scales.view(torch.int32))
    if base is not None:
        assert torch.equal(base.cpu().view(torch.int32), (b0 + sign.dequantize_tensor(bits, scales, d.shape)).view(torch.int32))


def run(P, rounds, res):
    from flame_amd import engine, sign
    dev = torch.device("cuda", 0)
    w = torch.empty(P, dtype=torch.float32, device=dev)
    engine.synth_fill_(w, 7, 0, 0, 1.0)
    for with_base in (False, True):
        tag = f"{P // 1_000_000}M/{'base' if with_base else 'plain'}"
        nbase, tbase = (torch.empty_like(w), torch.empty_like(w)) if with_base else (None, None)
        if with_base:
            engine.synth_fill_(nbase, 7, 1, 0, 1.0)
            tbase.copy_(nbase)
        _check(engine, sign, w, nbase)
        per = 12 if with_base else 4                    # bytes the launch moves per element, the 0.14 out aside
        src = torch.empty(per * P // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        kernel = []

        def native():
            engine.kernel_events = []
            out = engine.sign_compress({"model": w}, base={"model": nbase} if with_base else None)
            evs, engine.kernel_events = engine.kernel_events, None
            assert len(evs) == 1 and evs[0][0] == "flame_onebit_pack", evs
            kernel.append(evs[0])
            return out

        def torch_ops():
            if not with_base:
                return sign.compress({"model": w})
            out = sign.compress({"model": w - tbase})
            tbase.add_(sign.dequantize(out)["model"])
            return out
        arms = [("copy", lambda: dst.copy_(src)), ("native", native), ("torch", torch_ops)]
        times = {nm: [] for nm, _ in arms}
        for r in range(rounds + 1):                     # round 0 warms up
            for nm, fn in (arms if r % 2 == 0 else arms[::-1]):
                torch.cuda.synchronize()
                ms, out = _events(fn)
                torch.cuda.synchronize()
                del out
                if r:
                    times[nm].append(ms)
        c_ms, n_ms, t_ms = (statistics.median(times[nm]) for nm in ("copy", "native", "torch"))
        k_ms = statistics.median(e0.elapsed_time(e1) for _, e0, e1, _ in kernel[-rounds:])
        _line(res, f"{tag}/copy", times["copy"], GBps=round(per * P / c_ms / 1e6, 1))
        _line(res, f"{tag}/native", times["native"], kernel_ms=round(k_ms, 4), kernel_GBps=round(per * P / k_ms / 1e6, 1),
              kernel_x_copy=round(k_ms / c_ms, 3), launcher_ms=round(n_ms - k_ms, 4))
        _line(res, f"{tag}/torch", times["torch"], x_native=round(t_ms / n_ms, 2))
        del src, dst, nbase, tbase


def main():
    global _LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "sign_pack_rate.log"))
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    torch.empty(1, device="cuda:0")
    _LOG = open(a.log, "w")
    if not a.no_settle:
        import bench
        _say("settle: " + json.dumps(bench.settle_hbm(max_s=10.0)))
    res = {}
    for P in SHAPES:
        run(P, a.rounds, res)
    _say(json.dumps({"metric": "sign_pack_rate", "rounds": a.rounds, "arms": res}))


if __name__ == "__main__":
    main()
