"""Generate ``fedavg_clipped.npz`` by running the REAL reference: its own
``DifferentialPrivacy._apply_clip_norm_torch`` (privacy/differential_privacy.py:63-84) on every
client's update, then its ``FedAvg.do`` over the clipped updates.

Run in the build container only (the reference never travels), like make_golden.py:

    PYTHONPATH=tests/golden/_shim:<reference>/lib/python PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/make_golden_guard.py

Shape: 6 clients, an f32 and a bf16 key, 3 clients above the threshold, none within 1e-3
(relative) of it -- asserted below.  Besides the inputs and the reference's model the fixture
stores the reference's fp32 ``total_norm`` and scale per client and ``norm_tol``: 4 x the largest
relative difference between the reference's ``total_norm`` and the exact (``math.fsum``) norm over
these clients, measured when the fixture is made (torch's fp32 reduction order varies with the
host's vector width, hence the factor; the bf16 key's own norm is rounded to bf16 by torch.norm).
"""
from __future__ import annotations

import math
import os
import sys
from copy import deepcopy

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fixture_io import FixtureWriter  # noqa: E402

from flame.optimizers import optimizer_provider  # noqa: E402  (reference, via PYTHONPATH)
from flame.optimizer.train_result import TrainResult  # noqa: E402
from flame.privacy.differential_privacy import DifferentialPrivacy  # noqa: E402
from diskcache import Cache  # noqa: E402  (shim)

torch.set_num_threads(1)

CLIP = 4.0
N = 6
SHAPES = {"w": ((16, 16), torch.float32), "h": ((32,), torch.bfloat16)}
# per-client spread of the update: norms from well below to well above CLIP
SIGMA = [0.05, 0.6, 0.1, 0.45, 0.2, 0.33]


def exact_norm(w) -> float:
    terms = []
    for v in w.values():
        x = v.double().reshape(-1)
        terms.extend((x * x).tolist())
    return math.sqrt(math.fsum(terms))


class _Watch:
    """Stands in for the ``torch`` module the reference object holds (``dp.torch``): every call goes
    to torch unchanged; the values the reference's own statements produced are kept -- what its
    ``norm`` calls returned (the last one per update is its ``total_norm``) and the scale it handed
    to ``mul``."""

    def __init__(self):
        self.norms, self.scales = [], []

    def norm(self, *a, **k):
        r = torch.norm(*a, **k)
        self.norms.append(r)
        return r

    def mul(self, x, other, *a, **k):
        self.scales.append(other)
        return torch.mul(x, other, *a, **k)

    def __getattr__(self, name):
        return getattr(torch, name)


def main():
    gen = torch.Generator().manual_seed(2024)
    base = {k: torch.randn(s, generator=gen, dtype=torch.float64).to(dt) for k, (s, dt) in SHAPES.items()}
    clients = [{k: (torch.randn(s, generator=gen, dtype=torch.float64) * SIGMA[i]).to(dt)
                for k, (s, dt) in SHAPES.items()} for i in range(N)]
    counts = [17, 5, 40, 11, 23, 8]
    ids = [f"end{i:02d}" for i in range(N)]
    dp = DifferentialPrivacy(clip_threshold=CLIP, noise_factor=0.0)
    ref_norm, ref_scale, clipped, rel = [], [], [], []
    for w in clients:
        dp.torch = watch = _Watch()
        out = dp._apply_clip_norm_torch(w, CLIP)
        tn = watch.norms[-1]                      # the reference's total_norm, from its own call
        was = out is not w
        assert len(watch.norms) == len(w) + 1 and len(watch.scales) == (len(w) if was else 0)
        assert all(float(s) == float(watch.scales[0]) for s in watch.scales)
        ref_norm.append(float(tn))
        ref_scale.append(float(watch.scales[0]) if was else 1.0)     # the scale it multiplied by
        clipped.append(out)
        ex = exact_norm(w)
        rel.append(abs(float(tn) - ex) / ex)
        assert abs(ex - CLIP) / CLIP > 1e-3, "a client within 1e-3 of the threshold"
        assert (ex > CLIP) == was
    assert sum(s != 1.0 for s in ref_scale) == 3
    norm_tol = 4 * max(rel)
    print("largest relative difference reference total_norm vs fsum:", max(rel), "norm_tol:", norm_tol)
    cache = Cache()
    for e, w, c in zip(ids, clipped, counts):
        cache[e] = TrainResult(w, c)
    order = list(cache.iterkeys())
    model = optimizer_provider.get("fedavg").do(deepcopy(base), cache, total=sum(counts), num_trainers=N)
    fw = FixtureWriter()
    fw.meta.update({"kind": "fedavg_clipped", "n": N, "end_ids": ids, "order": order, "counts": counts,
                    "clip_threshold": CLIP, "norm_tol": norm_tol, "norm_rel_diff_max": max(rel),
                    "ref_total_norm": ref_norm, "ref_scale": ref_scale})
    fw.put_weights("base", base)
    for i, w in enumerate(clients):
        fw.put_weights(f"client{i}", w)
    fw.put_weights("out", model)
    fw.save(os.path.join(HERE, "fedavg_clipped.npz"))
    print("wrote fedavg_clipped.npz")


if __name__ == "__main__":
    main()
