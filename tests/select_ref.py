"""Test-side restatement of the trimmed mean by selection (include/flame_amd.h:
flame_agg_select) in numpy / torch-CPU, on tests/trimmed_ref.py's keys and order.

Per element, with ``s = sorted(keys)``: ``lo = s[k]``, ``hi = s[n - k - 1]`` (taken by ``np.sort``);
the values strictly between them are added in fp64 in CLIENT order to an accumulator that starts at
+0.0; then ``double(c_lo) * widen(value(lo))`` is added (one fp64 multiply, one fp64 add), where
``c_lo = #{key <= lo} - k``, and, if ``lo != hi``, ``double(c_hi) * widen(value(hi))`` with
``c_hi = #{key >= hi} - k``.  If ``lo == hi`` the one term carries ``c_lo = n - 2k``.  The mean,
its rounding and ``base + mean`` are ``trimmed_ref.finish``.
"""
import numpy as np

import trimmed_ref as R


def select(xs, k: int, base, dtype):
    """The restatement over ``xs`` (the ``n`` updates' flattened tensors for one key, in cache
    order); ``base`` None is FLAME_AGG_INIT_FIRST.  Returns a 1-D tensor."""
    n = len(xs)
    assert 0 <= k and 2 * k < n
    keys = np.stack([R.to_key(R.bits(x), dtype) for x in xs])
    srt = np.sort(keys, axis=0)
    lo, hi = srt[k], srt[n - k - 1]
    acc = np.zeros(keys.shape[1], np.float64)            # +0.0
    with np.errstate(all="ignore"):
        for i in range(n):
            inside = (lo < keys[i]) & (keys[i] < hi)
            acc = np.where(inside, acc + R.widen(keys[i], dtype), acc)
        one = lo == hi
        c_lo = np.where(one, n - 2 * k, (keys <= lo).sum(0) - k).astype(np.float64)
        c_hi = ((keys >= hi).sum(0) - k).astype(np.float64)
        assert (c_lo >= 1).all() and (c_hi >= 1).all()
        acc = acc + c_lo * R.widen(lo, dtype)
        acc = np.where(one, acc, acc + c_hi * R.widen(hi, dtype))
    return R.finish(acc, n - 2 * k, base, dtype)


def radix_order_statistic(keys: np.ndarray, rank: int, bits: int, digit: int = 4) -> np.ndarray:
    """The kernel's search, restated: ``sorted(keys, axis=0)[rank]`` per column by MSB-first digit
    passes -- count the digits of the keys that carry the prefix found so far, take the digit at
    which the running count crosses the rank.  ``keys`` is [n, numel] unsigned."""
    ut = keys.dtype.type
    prefix = np.zeros(keys.shape[1], keys.dtype)             # right-aligned
    r = np.full(keys.shape[1], rank, np.int64)
    for shift in range(bits - digit, -1, -digit):
        hb = keys >> ut(shift)
        match = (hb >> ut(digit)) == prefix
        d = (hb & ut((1 << digit) - 1)).astype(np.int64)
        hist = np.stack([(match & (d == b)).sum(0) for b in range(1 << digit)])      # [bins, numel]
        cum = np.cumsum(hist, axis=0)
        below = cum <= r                                     # a prefix of the bins, the counts being >= 0
        dig = below.sum(0)
        assert (dig < (1 << digit)).all()
        r = r - np.where(below, cum, 0).max(0)
        prefix = (prefix << ut(digit)) | dig.astype(keys.dtype)
    return prefix
