"""The geometric-median rule (RFA, smoothed Weiszfeld) restated independently of
flame_amd/optimizer/rfa.py, in numpy fp64 and ``math.fsum`` on the CPU ("The RFA
contract"), and the distance statement of ``flame_update_dist`` (include/flame_amd.h).

* :func:`dist2`: per update ``sum_e t(e)``, ``t = 0`` and a count for a non-finite ``x[e]``, else
  ``(fp64(x[e]) - fp64(z[e]))^2`` -- the terms are formed in fp64 and added by ``math.fsum``, so the
  sum itself is correctly rounded.
* :func:`weights`: ``w_i = beta_i / fsum(beta)``, ``beta_i = 1 / max(nu, sqrt(D_i))``, 0 for a
  ``D_i`` that is ``+inf`` or NaN; the previous weights when every ``beta`` is 0.
* :func:`geomedian`: the iteration on fp64 vectors with an fp64 centre.

Also here: the collusion round the CPU and GPU tests share.
"""
import math

import numpy as np
import torch


def _f64(t):
    return t.detach().cpu().to(torch.float64).reshape(-1).numpy()


def float_keys(update):
    return [k for k in update.keys() if isinstance(update[k], torch.Tensor) and update[k].is_floating_point()]


def dist2(ups, center):
    """``(dist2: list of float, nonfinite: list of int)`` of the updates ``ups`` (dicts of tensors)
    to ``center`` (a dict holding every float key), over each update's own float keys."""
    out, bad = [], []
    for u in ups:
        terms, nb = [], 0
        for k in float_keys(u):
            x, z = _f64(u[k]), _f64(center[k])
            fin = np.isfinite(x)
            nb += int((~fin).sum())
            with np.errstate(over="ignore", invalid="ignore"):
                d = np.where(fin, x, 0.0) - np.where(fin, z, 0.0)
                terms.extend((d * d).tolist())
        if any(math.isnan(t) for t in terms):
            out.append(math.nan)
        elif any(math.isinf(t) for t in terms):
            out.append(math.inf)
        else:
            try:
                out.append(math.fsum(terms))
            except OverflowError:
                out.append(math.inf)
        bad.append(nb)
    return out, bad


def weights(d2, nu, previous):
    beta = []
    for d in d2:
        d = float(d)
        beta.append(0.0 if (math.isnan(d) or math.isinf(d)) else 1.0 / max(nu, math.sqrt(d)))
    total = math.fsum(beta)
    if total == 0.0:
        return list(previous)
    return [b / total for b in beta]


def geomedian(xs, T, nu=1e-6):
    """``T`` smoothed Weiszfeld iterations from the centre 0 over the fp64 vectors ``xs``.  Returns
    ``(weights, trace)``, ``trace`` holding one ``(dist2, weights)`` per iteration."""
    xs = [np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]
    n = len(xs)
    w, z, trace = [1.0 / n] * n, np.zeros_like(xs[0]), []
    for t in range(1, T + 1):
        d2 = [math.fsum(((x - z) ** 2).tolist()) for x in xs]
        w = weights(d2, nu, w)
        trace.append((tuple(d2), tuple(w)))
        if t < T:
            z = np.sum([wi * x for wi, x in zip(w, xs)], axis=0)
    return w, trace


def combine(xs, w):
    return np.sum([wi * np.asarray(x, dtype=np.float64) for wi, x in zip(w, xs)], axis=0)


# ---------------------------------------------------------------------------- the shared attack
def bad_positions(n, bad):
    """``bad`` cache positions spread over the round."""
    return sorted({(2 + (i * n) // bad) % n for i in range(bad)})


def attack_round(gen, n, bad, numel=4099):
    """``n`` fp32 updates of ``numel`` elements: honest ones ``mu + N(0, (2e-3)^2)`` around one
    ``mu ~ N(0, (1e-2)^2)``, ``bad`` colluders ``-4 mu + N(0, (1e-4)^2)``.  Returns ``(updates as fp32
    tensors, colluder positions, the honest updates' fp64 mean)``."""
    mu = 1e-2 * torch.randn(numel, generator=gen, dtype=torch.float64)
    pos = bad_positions(n, bad)
    assert len(pos) == bad
    ups = []
    for i in range(n):
        if i in pos:
            x = -4.0 * mu + 1e-4 * torch.randn(numel, generator=gen, dtype=torch.float64)
        else:
            x = mu + 2e-3 * torch.randn(numel, generator=gen, dtype=torch.float64)
        ups.append(x.to(torch.float32))
    honest = np.mean([_f64(u) for i, u in enumerate(ups) if i not in pos], axis=0)
    return ups, pos, honest
