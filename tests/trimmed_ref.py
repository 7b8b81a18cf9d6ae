"""Test-side restatement of the coordinate-wise trimmed mean (include/flame_amd.h:
flame_agg_trimmed) in numpy / torch-CPU.  Two independent routes to the same statement:

* :func:`stream` -- the streaming procedure itself, vectorised over elements: a Python loop over
  clients and chain stages with ``np.minimum`` / ``np.maximum`` on the integer keys, the kept
  values added in fp64 in the order they emerge.  The GPU kernel is compared with this bitwise.
* :func:`by_sort` -- the definition: sort the keys, take ``[k : n - k]``, add ascending.  Equal to
  :func:`stream` bit for bit whenever the fp64 sum is exact (then the order cannot matter).

Order: ``-inf < .. < -0 < +0 < .. < +inf < NaN``, all NaNs equal and largest (``torch.sort``'s
placement).  Key: the bit pattern with the sign bit flipped for non-negative values and all bits
flipped for negative ones, at the dtype's width; every NaN maps to the all-ones key.
"""
import numpy as np
import torch

_U = {torch.float32: (np.uint32, torch.int32, 32, 0x7F800000),
      torch.bfloat16: (np.uint16, torch.int16, 16, 0x7F80),
      torch.float16: (np.uint16, torch.int16, 16, 0x7C00),
      torch.float64: (np.uint64, torch.int64, 64, 0x7FF0000000000000)}


def bits(t: torch.Tensor) -> np.ndarray:
    """The bit patterns of a float tensor as an unsigned numpy array (flattened)."""
    ut, it, _, _ = _U[t.dtype]
    return t.detach().cpu().contiguous().reshape(-1).view(it).numpy().view(ut).copy()


def from_bits(u: np.ndarray, dtype) -> torch.Tensor:
    ut, it, _, _ = _U[dtype]
    return torch.from_numpy(np.ascontiguousarray(u, dtype=ut)).view(it).view(dtype)


def to_key(u: np.ndarray, dtype) -> np.ndarray:
    ut, _, w, inf = _U[dtype]
    top = ut(1 << (w - 1))
    ones = ut((1 << w) - 1)
    u = u.astype(ut)
    key = u ^ np.where((u >> ut(w - 1)) != 0, ones, top).astype(ut)
    key[(u & ut(ones ^ top)) > ut(inf)] = ones
    return key


def from_key(key: np.ndarray, dtype) -> np.ndarray:
    ut, _, w, _ = _U[dtype]
    top = ut(1 << (w - 1))
    ones = ut((1 << w) - 1)
    key = key.astype(ut)
    return key ^ np.where((key >> ut(w - 1)) != 0, top, ones).astype(ut)     # all ones -> 0x7f..f, a quiet NaN


def widen(key: np.ndarray, dtype) -> np.ndarray:
    """Keys decoded and widened to fp64 (exact for every dtype)."""
    return from_bits(from_key(key, dtype), dtype).double().numpy()


def finish(acc: np.ndarray, kept: int, base, dtype) -> torch.Tensor:
    """mean64 = acc / kept (one fp64 division), rounded to the dtype (f32: one RNE step; bf16 / f16:
    fp64 -> fp32 -> 16 bit), then ``base + mean`` as one torch-CPU add in the dtype (or the mean)."""
    with np.errstate(all="ignore"):
        mean64 = acc / np.float64(kept)
        if dtype == torch.float64:
            mean = torch.from_numpy(mean64.copy())
        else:
            mean = torch.from_numpy(mean64.astype(np.float32))
            if dtype != torch.float32:
                mean = mean.to(dtype)
    if base is None:
        return mean
    return base.detach().cpu().reshape(-1) + mean


def _keys(xs, dtype):
    return [to_key(bits(x), dtype) for x in xs]


def stream(xs, k: int, base, dtype) -> torch.Tensor:
    """The streaming selection of DESIGN.md §2 over ``xs`` (the ``n`` updates' flattened tensors
    for one key, in cache order); ``base`` None is FLAME_AGG_INIT_FIRST.  Returns a 1-D tensor."""
    n = len(xs)
    assert 0 <= k and 2 * k < n
    keys = _keys(xs, dtype)
    lo, hi = [], []
    acc = np.zeros(keys[0].shape, np.float64)            # +0.0
    for i, x in enumerate(keys):
        x = x.copy()
        if i < k:                                        # arrivals 0 .. k-1: insertion-sorted into lo
            for j in range(len(lo)):
                lo[j], x = np.minimum(lo[j], x), np.maximum(lo[j], x)
            lo.append(x)
            continue
        for j in range(k):                               # through lo: what emerges is not among the k smallest
            lo[j], x = np.minimum(lo[j], x), np.maximum(lo[j], x)
        if i < 2 * k:                                    # arrivals k .. 2k-1: insertion-sorted into hi
            for j in range(len(hi)):
                hi[j], x = np.maximum(hi[j], x), np.minimum(hi[j], x)
            hi.append(x)
            continue
        for j in range(k):                               # through hi: what emerges is kept
            hi[j], x = np.maximum(hi[j], x), np.minimum(hi[j], x)
        with np.errstate(all="ignore"):
            acc = acc + widen(x, dtype)                  # one IEEE fp64 add, in emergence order
    return finish(acc, n - 2 * k, base, dtype)


def by_sort(xs, k: int, base, dtype) -> torch.Tensor:
    """The definition: sorted(x)[k : n - k], added ascending in fp64."""
    n = len(xs)
    assert 0 <= k and 2 * k < n
    srt = np.sort(np.stack(_keys(xs, dtype)), axis=0)
    acc = np.zeros(srt.shape[1], np.float64)
    with np.errstate(all="ignore"):
        for i in range(k, n - k):
            acc = acc + widen(srt[i], dtype)
    return finish(acc, n - 2 * k, base, dtype)


def exact_inputs(g, dt, n, numel):
    """``n`` tensors whose every partial sum is exact in fp64: m * 2^-24 with integer |m| < 2^24
    (f32 / f64), integers in [-8, 8] (bf16 / f16)."""
    if dt in (torch.float32, torch.float64):
        return [(torch.randint(-(2 ** 24) + 1, 2 ** 24, (numel,), generator=g).double() * 2.0 ** -24).to(dt)
                for _ in range(n)]
    return [torch.randint(-8, 9, (numel,), generator=g).to(dt) for _ in range(n)]


def same_bits(label, got: torch.Tensor, want: torch.Tensor) -> None:
    """Bitwise equality; a NaN matches any NaN (sign and payload are not pinned)."""
    got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    bad = (gn != wn) | (~gn & (torch.from_numpy(bits(got) != bits(want))))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {got.numel()} elements differ, first at {i}: "
                             f"got {got[i].item()!r} (0x{int(bits(got)[i]):x}), want {want[i].item()!r} "
                             f"(0x{int(bits(want)[i]):x})")
