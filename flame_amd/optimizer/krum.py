"""The ``krum`` kwarg: Krum / Multi-Krum selection in front of the weighted average (Blanchard,
El Mhamdi, Guerraoui, Stainer, NeurIPS 2017, "Machine Learning with Adversaries: Byzantine
Tolerant Gradient Descent"; flame has no counterpart -- its ``OptimizerType`` is a closed enum, so
the reachable form is a kwarg of the existing classes, like the update guard's and ``trim``).

The update guard bounds an update's *norm* and ``trim`` drops per-coordinate outliers; both look at
one update at a time.  Krum looks at the updates *relative to each other*: an update is scored by
the sum of its squared distances to its ``q = n - f - 2`` nearest neighbours, and the ``m`` lowest
scores are averaged with equal weights.  A colluding minority of at most ``f`` updates that keeps
a plausible norm and shifts every coordinate a little is far from the honest majority's cluster
and is not selected.

``krum`` is ``None`` (the default: nothing here runs), an int ``f >= 0`` (the assumed number of
bad updates) or a float fraction in ``[0, 0.5)`` (``f = floor(krum * n)``).  ``krum_select`` is
``None`` (``m = n - f``: Multi-Krum) or an int ``>= 1`` (``1`` is Krum).  A round needs
``n >= 2f + 3``.  ``count`` and ``total`` play no part: a count-weighted Multi-Krum would let a
liar choose its own weight.

The device measures one thing, the Gram matrix ``G[i][j] = sum_e s(x_i[e]) s(x_j[e])`` over the
sanitised float elements (``engine.update_gram``, kernel ``flame_update_gram``); everything below
is host arithmetic in fp64.  The statement is in DESIGN.md §2 ("The Krum contract").
"""
import collections
import math

import numpy as np

from .. import metrics

KrumRecord = collections.namedtuple("KrumRecord", "end norm nonfinite score selected")


def check_kwargs(krum, krum_select):
    """Validate the two constructor kwargs; returns them (a fraction as float, counts as int)."""
    if krum is None:
        if krum_select is not None:
            raise ValueError("krum_select needs krum (the assumed number of bad updates)")
        return None, None
    if isinstance(krum, bool):
        raise TypeError("krum must be None, an int >= 0 or a float in [0, 0.5), not a bool")
    if isinstance(krum, int):
        if krum < 0:
            raise ValueError(f"krum must be >= 0, not {krum!r}")
    elif isinstance(krum, float):
        if not (0.0 <= krum < 0.5):          # a NaN fails both
            raise ValueError(f"krum as a fraction must lie in [0, 0.5), not {krum!r}")
    else:
        raise TypeError(f"krum must be None, an int >= 0 or a float in [0, 0.5), not {type(krum).__name__}")
    if krum_select is not None:
        if isinstance(krum_select, bool) or not isinstance(krum_select, int):
            raise TypeError(f"krum_select must be None or an int >= 1, not {type(krum_select).__name__}")
        if krum_select < 1:
            raise ValueError(f"krum_select must be >= 1, not {krum_select!r}")
    return krum, krum_select


def count(krum, n: int) -> int:
    """The assumed number of bad updates ``f`` of a round of ``n`` updates."""
    if isinstance(krum, float):
        return int(math.floor(krum * n))
    return int(krum)


def check_round(krum, krum_select, n: int, max_clients: int):
    """``(f, q, m)`` for ``n`` updates, or the round's refusal: NotImplementedError when ``n``
    exceeds the Gram kernel's client capacity, ValueError when ``n < 2f + 3`` (Blanchard et al.)
    or ``krum_select > n - f``."""
    if n > max_clients:
        raise NotImplementedError(
            f"flame_amd krum={krum!r}: {n} updates exceed the Gram kernel's capacity of {max_clients} "
            "(flame_update_gram_max_clients); a larger round is a follow-up (DESIGN.md §8)")
    f = count(krum, n)
    if n < 2 * f + 3:
        raise ValueError(f"flame_amd krum={krum!r}: f = {f} needs at least 2f + 3 = {2 * f + 3} updates, "
                         f"the round has {n}")
    m = n - f if krum_select is None else int(krum_select)
    if m > n - f:
        raise ValueError(f"flame_amd krum_select={krum_select!r}: at most n - f = {n - f} of {n} updates can be "
                         f"selected with f = {f}")
    return f, n - f - 2, m


def distances(gram, nonfinite, scales):
    """``d[i][j] = max(0, (a_i + a_j) - 2 (s_i s_j G[i][j]))`` with ``a_i = s_i^2 G[i][i]``, fp64;
    ``+inf`` to and from an ineligible update (non-finite elements, or a non-finite ``G[i][i]``).
    Returns ``(d, eligible)``; the diagonal is 0 (``+inf`` for an ineligible update)."""
    g = np.asarray(gram, dtype=np.float64)
    n = g.shape[0]
    s = np.ones(n, np.float64) if scales is None else np.asarray(scales, dtype=np.float64)
    diag = np.diagonal(g)
    eligible = (np.asarray(nonfinite, dtype=np.int64) == 0) & np.isfinite(diag)
    with np.errstate(invalid="ignore", over="ignore"):
        a = s * s * diag
        d = np.maximum(0.0, (a[:, None] + a[None, :]) - 2.0 * (s[:, None] * s[None, :] * g))
    d[~np.isfinite(d)] = np.inf             # a NaN from an overflowed f64 product counts as infinitely far
    d[~eligible, :] = np.inf
    d[:, ~eligible] = np.inf
    return d, eligible


def select(gram, nonfinite, scales, f: int, m: int):
    """Scores and selection of one round.  ``score_i`` is ``math.fsum`` of the ``q = n - f - 2``
    smallest ``d[i][j]``, ``j != i`` (``+inf`` if any of them is); the ``m`` smallest finite
    scores are selected, ties to the earlier position, fewer if fewer are finite.  Returns
    ``(scores: list of float, selected: sorted list of indices)``."""
    d, _ = distances(gram, nonfinite, scales)
    n = d.shape[0]
    q = n - f - 2
    scores = []
    for i in range(n):
        near = np.sort(np.delete(d[i], i))[:q]
        scores.append(math.inf if np.isinf(near).any() else math.fsum(near))
    order = sorted((i for i in range(n) if math.isfinite(scores[i])), key=lambda i: scores[i])     # stable
    return scores, sorted(order[:m])


def records(ends, gram, nonfinite, scores, selected):
    chosen = set(selected)
    return [KrumRecord(end, math.sqrt(float(gram[i][i])) if gram[i][i] >= 0 else math.nan, int(nonfinite[i]),
                       scores[i], i in chosen) for i, end in enumerate(ends)]


def save_metrics(owner, recs, f: int) -> None:
    """``krum_selected`` / ``krum_f`` / ``krum_score_max`` (over the finite scores) beside the kernel metrics."""
    mc, alias = metrics.collector(owner)
    if mc is None or not recs:
        return
    finite = [r.score for r in recs if math.isfinite(r.score)]
    mc.save("krum_selected", alias, sum(1 for r in recs if r.selected))
    mc.save("krum_f", alias, f)
    mc.save("krum_score_max", alias, max(finite) if finite else math.nan)
