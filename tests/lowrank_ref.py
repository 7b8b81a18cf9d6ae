"""The low-rank contract in numpy fp64.  A plain module, no tests."""
import numpy as np


def accumulate(base, updates, rates):
    """``base`` (fp32 [m, n]) after ``updates``, ``[(U [m, r], V [r, n])]`` in client order (fp32 arrays): ``(exact, mag)``, the fp64
    sum over the fp32-rounded scaled left factors and the per-element ``|in| + sum |f32(u * rate)| |v|`` of the error bound."""
    exact = np.asarray(base, dtype=np.float64).copy()
    mag = np.abs(exact)
    with np.errstate(all="ignore"):
        for (u, v), r in zip(updates, rates):
            us = (np.asarray(u, dtype=np.float32) * np.float32(r)).astype(np.float32).astype(np.float64)
            exact += us @ np.asarray(v, dtype=np.float64)
            mag += np.abs(us) @ np.abs(np.asarray(v, dtype=np.float64))
    return exact, mag


def gamma(k):       # gamma_k = k 2^-24 / (1 - k 2^-24), the error factor of an fp32 sum of k terms in any order
    return k * 2.0 ** -24 / (1 - k * 2.0 ** -24)
