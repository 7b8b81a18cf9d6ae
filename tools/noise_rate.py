#!/usr/bin/env python3
"""What server-side noise (``noise_factor``) costs, in ONE process, after the bench's HBM settling, the
arms interleaved round by round in alternating order and each checked against the others:

  the fill alone (HIP-event kernel time, engine.kernel_events)
    engine.noise_fill over --params fp32 / bf16 elements -> flame_noise_fill (write-only), beside a
    same-size ``torch.Tensor.fill_`` as the write yardstick of the same buffer in the same process
  whole rounds (HIP events on the current stream around ``do()``) over one slab of --clients fp32 updates
    FedAvg.do  / FedAvg(noise_factor=s).do
    FedAdam.do / FedAdam(noise_factor=s).do      (adaptive rounds: state from a first round)
  host issue time (``time.perf_counter`` around ``do()``, the stream idle before and drained after)
    the same four optimizers, from the slab of --clients updates and from one of --many-clients updates
    of --many-params elements: where an extra entry that is not a slab slot could lose the slab fast path

The arm with the kwarg unset runs no line of the feature: it is the round as it was before the feature.
Checks, once, before anything is timed: two fills give equal bits; the noised FedAvg model is bitwise
the un-noised model plus ``engine.accumulate(model, [(noise, 1.0)])`` with the same seed and round.

    python tools/noise_rate.py                                  # 64 x 25M fp32, 1,024 x 1M for the issue time
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TR = collections.namedtuple("TR", "weights count version")


class Cache(collections.OrderedDict):
    """The two calls an optimizer makes on flame's cache."""

    def iterkeys(self):
        return iter(list(self.keys()))


def make_slab(engine, UpdateSlab, n, P, dev):
    slab = UpdateSlab({"model": torch.empty(P, dtype=torch.float32)}, capacity=n, device=dev)
    fill = torch.empty(P, dtype=torch.float32, device=dev)
    slots = []
    for i in range(n):
        engine.synth_fill_(fill, 7, 1 + i, 0, 1e-2)
        slots.append(slab.put({"model": fill}))
    engine.synth_fill_(fill, 7, 0, 0, 1.0)
    torch.cuda.synchronize()
    return slab, slots, fill


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--params", type=int, default=25_000_000)
    ap.add_argument("--many-clients", type=int, default=1024)
    ap.add_argument("--many-params", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--noise-factor", type=float, default=1e-3)
    ap.add_argument("--no-settle", action="store_true")
    a = ap.parse_args()
    from flame_amd import engine
    from flame_amd.optimizer import FedAdam, FedAvg, noise
    from flame_amd.slab import UpdateSlab
    dev = torch.device("cuda", 0)
    n, P, s, seed = a.clients, a.params, a.noise_factor, 1234 | 5678 << 32
    slab, slots, model0 = make_slab(engine, UpdateSlab, n, P, dev)
    slab_m, slots_m, model0_m = make_slab(engine, UpdateSlab, a.many_clients, a.many_params, dev)

    # ---- checks: equal fills; noised FedAvg == un-noised FedAvg + the same noise as one more update
    like = {"model": model0}
    z0, z1 = engine.noise_fill(like, seed, 0, 0.5), engine.noise_fill(like, seed, 0, 0.5)
    assert torch.equal(z0["model"], z1["model"]) and bool(torch.isfinite(z0["model"]).all())
    mean, var = float(z0["model"].double().mean()), float(z0["model"].double().var())
    assert abs(mean) * (P ** 0.5) / 0.5 <= 5 and abs(var / 0.25 - 1) * (P / 2) ** 0.5 <= 5, (mean, var)
    del z0, z1

    def cache_of(sl):
        return Cache((f"e{i:05d}", TR(w, 1, 0)) for i, w in enumerate(sl))
    plain, noised = FedAvg(), FedAvg(noise_factor=s, noise_seed=seed)
    a_plain, a_noised = {"model": model0.clone()}, {"model": model0.clone()}
    plain.do(a_plain, cache_of(slots), total=n)
    noised.do(a_noised, cache_of(slots), total=n)
    engine.accumulate(a_plain, [(engine.noise_fill(a_plain, seed, 0, noised.noise_std), 1.0)])
    torch.cuda.synchronize()
    assert torch.equal(a_plain["model"], a_noised["model"]), "noised FedAvg != FedAvg + the same noise"
    assert noised.noise_round == 1 and noised.noise_std == noise.std_of(s, [1.0 / n] * n)
    del a_plain, a_noised
    print("checks: fills repeat; FedAvg(noise_factor) == FedAvg + noise as a last update, bitwise", flush=True)

    if not a.no_settle:
        import bench
        print("settle:", json.dumps(bench.settle_hbm(max_s=10.0)), flush=True)

    # ---- arms
    bf = {"model": torch.empty(P, dtype=torch.bfloat16, device=dev)}
    yard = {torch.float32: torch.empty(P, dtype=torch.float32, device=dev), torch.bfloat16: bf["model"]}

    def yardstick(dt):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            yard[dt].fill_(1.0)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run

    def fill_of(lk):
        def run():
            engine.kernel_events = []
            engine.noise_fill(lk, seed, 3, 0.5)
            torch.cuda.synchronize()
            evs, engine.kernel_events = engine.kernel_events, None
            assert len(evs) == 1 and evs[0][0] == "flame_noise_fill", evs
            return evs[0][1].elapsed_time(evs[0][2])
        return run

    def prepared(opt, sl, model):
        """(optimizer, model dict) with FedAdam's first (passthrough) round done: every timed round is adaptive."""
        agg = {"model": model.clone()}
        if isinstance(opt, FedAdam):
            opt.do(agg, cache_of(sl), total=len(sl))
            opt.current_weights = {"model": agg["model"].clone()}
            opt.do(agg, cache_of(sl), total=len(sl))        # m_t / v_t exist from here on
        torch.cuda.synchronize()
        return opt, agg

    def round_of(opt, agg, sl, host=False):
        def run():
            cache = cache_of(sl)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            opt.do(agg, cache, total=len(sl))
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            return (t1 - t0) * 1e3 if host else e0.elapsed_time(e1)
        return run

    arms = [("fill_f32", fill_of(like)), ("torch_fill_f32", yardstick(torch.float32)),
            ("fill_bf16", fill_of(bf)), ("torch_fill_bf16", yardstick(torch.bfloat16))]
    for tag, kw in (("", {}), ("+noise", {"noise_factor": s, "noise_seed": seed})):
        for nm, cls in (("fedavg", FedAvg), ("fedadam", FedAdam)):
            opt, agg = prepared(cls(**kw), slots, model0)
            arms.append((f"{nm}{tag}", round_of(opt, agg, slots)))
            arms.append((f"issue{n}_{nm}{tag}", round_of(opt, agg, slots, host=True)))
            opt_m, agg_m = prepared(cls(**kw), slots_m, model0_m)
            arms.append((f"issue{a.many_clients}_{nm}{tag}", round_of(opt_m, agg_m, slots_m, host=True)))
    times = {nm: [] for nm, _ in arms}
    for r in range(a.rounds + 1):               # round 0 warms up
        for nm, fn in (arms if r % 2 == 0 else arms[::-1]):
            ms = fn()
            if r:
                times[nm].append(ms)
    med = {nm: statistics.median(ts) for nm, ts in times.items()}
    res = {"metric": "noise_rate", "clients": n, "params": P, "many_clients": a.many_clients,
           "many_params": a.many_params, "rounds": a.rounds, "noise_factor": s}
    for nm, _ in arms:
        ms = med[nm]
        res[nm] = {"ms_median": round(ms, 4), "ms_min": round(min(times[nm]), 4), "ms_max": round(max(times[nm]), 4)}
        tail = ""
        if nm.startswith("fill_"):
            isz = 4 if nm.endswith("f32") else 2
            yd = med["torch_" + nm]
            res[nm].update(write_GBps=round(P * isz / ms / 1e6, 1), of_torch_fill=round(yd / ms, 4))
            tail = f"{P * isz / ms / 1e6:8.1f} GB/s written, {100 * yd / ms:.1f} % of torch.fill_'s rate on the same buffer"
        elif nm.startswith("torch_fill"):
            isz = 4 if nm.endswith("f32") else 2
            tail = f"{P * isz / ms / 1e6:8.1f} GB/s written (the yardstick)"
        elif nm.endswith("+noise"):
            base = med[nm[:-len("+noise")]]
            res[nm].update(vs_unnoised=round(ms / base, 4))
            tail = f"x{ms / base:.4f} of the un-noised {'issue time' if nm.startswith('issue') else 'round'} ({base:.4f} ms)"
        print(f"{nm:26s} {ms:9.4f} ms  (min {min(times[nm]):.4f}, max {max(times[nm]):.4f})  {tail}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
