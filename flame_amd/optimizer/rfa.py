"""The ``rfa`` kwarg: the geometric median of the round's updates by smoothed Weiszfeld iterations
(RFA: Pillutla, Kakade, Harchaoui, "Robust Aggregation for Federated Learning", IEEE Transactions
on Signal Processing 70, 2022; flame has no counterpart -- its ``OptimizerType`` is a closed enum,
so the reachable form is a kwarg of the existing classes, like the update guard's, ``trim`` and
``krum``).

The guard looks at an update's norm, ``trim`` at each coordinate, ``krum`` at the updates relative
to each other through an ``n x n`` matrix that it caps at 1,024 updates.  The geometric median is
the robust rule whose cost is linear in ``n`` and has no cap; it drops nothing, needs no assumed
number of bad updates, and its breakdown point is 1/2: every update is kept and down-weighted by
its distance to the current centre.

``rfa`` is ``None`` (the default: nothing here runs) or an int ``T >= 1``, the number of Weiszfeld
iterations; ``rfa_nu`` (default ``1e-6``) is the smoothing floor ``nu > 0`` of the distances.
``count`` and ``total`` play no part: a count-weighted median lets a liar choose its own weight.

Over the eligible updates ``E`` (no non-finite element, a finite sum of squares), all in fp64 on
the host, with ``D`` the squared distances to the current centre -- first the unchanged global
model, ``z = 0``, so ``D_i`` is ``engine.update_stats``' ``sumsq_i``::

    for t = 1 .. T:
        beta_i = 1 / max(nu, sqrt(D_i))       (0 when D_i is +inf or NaN)
        w_i    = beta_i / fsum(beta)          (every beta 0: stop, keep the previous weights --
                                               at t = 1 the equal weights)
        if t < T:  z = sum_i w_i x_i          (the ordinary reduction, FLAME_AGG_INIT_FIRST, in cache
                                               order, into scratch tensors of each key's own dtype)
                   D = engine.update_dist(x_E, z)

The stage returns ``[(x_i, w_i)]``; the round's reduction (or the fused FedOPT round) applies them.
``rfa=1`` launches no new kernel: it is inverse-norm weighting.  The statement is in DESIGN.md §2
("The RFA contract").
"""
import collections
import math

import torch

from .. import engine, metrics

RfaRecord = collections.namedtuple("RfaRecord", "end norm nonfinite dist weight")
DEFAULT_NU = 1e-6


def check_kwargs(rfa, rfa_nu):
    """Validate the two constructor kwargs; returns ``(T, nu)`` (``(None, None)`` when unset)."""
    if rfa_nu is not None:
        if isinstance(rfa_nu, bool) or not isinstance(rfa_nu, (int, float)):
            raise TypeError(f"rfa_nu must be a float > 0, not {type(rfa_nu).__name__}")
        if not (rfa_nu > 0 and math.isfinite(rfa_nu)):          # a NaN fails the first
            raise ValueError(f"rfa_nu must be finite and > 0, not {rfa_nu!r}")
    if rfa is None:
        if rfa_nu is not None:
            raise ValueError("rfa_nu needs rfa (the number of Weiszfeld iterations)")
        return None, None
    if isinstance(rfa, bool) or not isinstance(rfa, int):
        raise TypeError(f"rfa must be None or an int >= 1, not {'a bool' if isinstance(rfa, bool) else type(rfa).__name__}")
    if rfa < 1:
        raise ValueError(f"rfa must be >= 1, not {rfa!r}")
    return rfa, float(DEFAULT_NU if rfa_nu is None else rfa_nu)


def weights(dist2, nu: float, previous):
    """One Weiszfeld weighting: ``w_i = beta_i / fsum(beta)``, ``beta_i = 1 / max(nu, sqrt(D_i))`` and 0
    for a ``D_i`` that is ``+inf`` or NaN; ``previous`` when every ``beta`` is 0."""
    beta = [1.0 / max(nu, math.sqrt(d)) if math.isfinite(d) else 0.0 for d in map(float, dist2)]
    s = math.fsum(beta)
    if s == 0.0:
        return list(previous)
    return [b / s for b in beta]


def centre(ws, w):
    """``z = sum_i w_i x_i`` over the float keys of the updates ``ws``: one FLAME_AGG_INIT_FIRST
    reduction per dtype, in the order given, into fresh device tensors of each key's own dtype (a
    key some updates lack is summed over those that carry it).  Returns ``{key: tensor}``."""
    device = engine._hip_device(None, "rfa", *ws)
    per = collections.OrderedDict()             # key -> (dtype, shape, client indices), first-seen order
    for ci, x in enumerate(ws):
        for k in x.keys():
            dt = engine.weight_dtype(x, k)
            if dt.is_floating_point:
                per.setdefault(k, (dt, tuple(engine.logical_shape(x, k)), []))[2].append(ci)
    z = {k: torch.empty(shape, dtype=dt, device=device) for k, (dt, shape, _) in per.items()}
    groups = collections.OrderedDict()          # normally one: every update carries every key
    for k, (_, _, cis) in per.items():
        groups.setdefault(tuple(cis), []).append(k)
    for cis, ks in groups.items():
        engine.reduce_([z[k] for k in ks], None, [[ws[ci][k] for ci in cis] for k in ks], [w[ci] for ci in cis],
                       init_first=True)
    return z


def iterate(ws, sumsq, T: int, nu: float):
    """``T`` smoothed Weiszfeld iterations over the eligible updates ``ws`` whose squared norms are
    ``sumsq``.  Returns ``(weights, dist2, trace)``: the final weights, the squared distances they
    were formed from, and one ``(dist2 tuple, weights tuple)`` per iteration run."""
    n = len(ws)
    w, d2, trace = [1.0 / n] * n, [float(s) for s in sumsq], []
    for t in range(1, T + 1):
        w = weights(d2, nu, w)
        trace.append((tuple(d2), tuple(w)))
        if t == T or not any(math.isfinite(d) for d in d2):     # every beta is 0: the previous weights stand
            break
        d2 = [float(d) for d in engine.update_dist(ws, centre(ws, w))[0]]
    return w, d2, trace


def records(ends, sumsq, nonfinite, eligible, dist2, w):
    """One RfaRecord per popped update in cache order; an update outside ``eligible`` has distance
    NaN and weight 0."""
    pos = {i: p for p, i in enumerate(eligible)}
    out = []
    for i, end in enumerate(ends):
        p = pos.get(i)
        norm = math.sqrt(float(sumsq[i])) if sumsq[i] >= 0 else math.nan
        dist = math.nan if p is None or math.isnan(dist2[p]) else math.sqrt(dist2[p])
        out.append(RfaRecord(end, norm, int(nonfinite[i]), dist, 0.0 if p is None else w[p]))
    return out


def save_metrics(owner, trace) -> None:
    """``rfa_iterations`` / ``rfa_weight_min`` / ``rfa_dist_max`` (over the finite distances) beside the kernel metrics."""
    mc, alias = metrics.collector(owner)
    if mc is None or not trace:
        return
    d2, w = trace[-1]
    finite = [math.sqrt(d) for d in d2 if math.isfinite(d)]
    mc.save("rfa_iterations", alias, len(trace))
    mc.save("rfa_weight_min", alias, min(w))
    mc.save("rfa_dist_max", alias, max(finite) if finite else math.nan)
