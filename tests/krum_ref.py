"""Krum / Multi-Krum restated independently of flame_amd/optimizer/krum.py, in numpy fp64 on the
CPU ("The Krum contract").

The distances are formed DIRECTLY, ``d_ij = sum_e (s_i x_i[e] - s_j x_j[e])^2`` over the sanitised
elements (finite ? x : 0) of every float key -- never through a Gram matrix -- so a test that
compares the two routes compares two different computations.  Scores are ``math.fsum`` of the
``q = n - f - 2`` smallest distances to the others; the selection is a stable sort of the finite
scores.  Also here: the honest-plus-bad rounds the CPU and GPU tests share.
"""
import math

import numpy as np
import torch


def flatten(update):
    """(the update's float elements in key order as one sanitised fp64 vector, its non-finite count)."""
    parts, bad = [], 0
    for k in update.keys():
        t = update[k]
        if not (isinstance(t, torch.Tensor) and t.is_floating_point()):
            continue
        x = t.detach().cpu().to(torch.float64).reshape(-1).numpy()
        fin = np.isfinite(x)
        bad += int((~fin).sum())
        parts.append(np.where(fin, x, 0.0))
    return (np.concatenate(parts) if parts else np.zeros(0)), bad


def distances(ups, scales=None):
    """``(d, nonfinite)``: the n x n matrix of squared distances between the (scaled) sanitised
    updates, ``+inf`` to and from an update that holds a non-finite element or whose own sum of
    squares is not finite."""
    flat = [flatten(u) for u in ups]
    n = len(flat)
    s = [1.0] * n if scales is None else [float(x) for x in scales]
    with np.errstate(over="ignore", invalid="ignore"):
        xs = [v * s[i] if s[i] != 1.0 else v for i, (v, _) in enumerate(flat)]
        ok = [bad == 0 and bool(np.isfinite(np.dot(v, v))) for v, bad in flat]
        d = np.full((n, n), np.inf)
        for i in range(n):
            if not ok[i]:
                continue
            for j in range(i, n):
                if ok[j]:
                    diff = xs[i] - xs[j]
                    v = float(np.dot(diff, diff))
                    d[i, j] = d[j, i] = v if math.isfinite(v) else np.inf
    return d, np.asarray([bad for _, bad in flat], np.int64)


def scores(d, f):
    n = d.shape[0]
    q = n - f - 2
    out = []
    for i in range(n):
        near = sorted(float(d[i, j]) for j in range(n) if j != i)[:q]
        out.append(math.inf if any(math.isinf(x) for x in near) else math.fsum(near))
    return out


def select(d, f, m=None):
    """``(scores, selected indices in cache order)``; ``m`` defaults to ``n - f`` (Multi-Krum)."""
    n = d.shape[0]
    sc = scores(d, f)
    m = n - f if m is None else m
    order = sorted([i for i in range(n) if math.isfinite(sc[i])], key=lambda i: sc[i])       # stable
    return sc, sorted(order[:m])


def krum(ups, f, m=None, scales=None):
    d, nf = distances(ups, scales)
    sc, sel = select(d, f, m)
    return sc, sel, d, nf


# ---------------------------------------------------------------------------- shared rounds
def bad_positions(n, f):
    """``f`` cache positions spread over the round (never two rules for one position)."""
    return sorted({(3 + (i * n) // max(f, 1)) % n for i in range(f)}) if f else []


def honest_bad(gen, n, f, sizes, dtype=torch.float32):
    """A round of ``n`` updates over keys ``k0, k1, ..`` of ``sizes`` elements: ``n - f`` honest ones
    ``g + 0.1 N(0, 1)`` around one ``g ~ N(0, 1)`` per element, and ``f`` bad ones cycling through a
    sign-flipped honest draw, an honest draw x 8, ``3 N(0, 1) + 1`` and an honest draw ``+ 2.0``.
    Returns ``(updates, honest positions)``."""
    g = {f"k{j}": torch.randn(s, generator=gen, dtype=torch.float64) for j, s in enumerate(sizes)}
    bad = bad_positions(n, f)
    assert len(bad) == f
    ups, kind = [], 0
    for i in range(n):
        h = {k: v + 0.1 * torch.randn(v.shape, generator=gen, dtype=torch.float64) for k, v in g.items()}
        if i in bad:
            rule = kind % 4
            kind += 1
            if rule == 0:
                h = {k: -v for k, v in h.items()}
            elif rule == 1:
                h = {k: 8.0 * v for k, v in h.items()}
            elif rule == 2:
                h = {k: 3.0 * torch.randn(v.shape, generator=gen, dtype=torch.float64) + 1.0 for k, v in h.items()}
            else:
                h = {k: v + 2.0 for k, v in h.items()}
        ups.append({k: v.to(dtype) for k, v in h.items()})
    return ups, [i for i in range(n) if i not in bad]


def integer_updates(gen, n, sizes, dtype=torch.float32, lo=-8, hi=8):
    """``n`` different updates of integers in [lo, hi]: every product and partial sum of a Gram
    matrix or a squared distance over them is exact in fp64, in any order."""
    return [{f"k{j}": torch.randint(lo, hi + 1, (s,), generator=gen).to(dtype) for j, s in enumerate(sizes)}
            for _ in range(n)]


def exact_gram(ups):
    """The Gram matrix of integer-valued updates, exact: every product and every partial sum is an
    integer below 2^53, so the fp64 matrix product is exact in any order (asserted)."""
    x = np.stack([np.concatenate([u[k].detach().cpu().to(torch.float64).reshape(-1).numpy()
                                  for k in u.keys() if u[k].is_floating_point()]) for u in ups])
    assert np.array_equal(np.rint(x), x)
    assert float((np.abs(x).max(initial=0.0) ** 2) * max(x.shape[1], 1)) < 2.0 ** 53
    return x @ x.T
