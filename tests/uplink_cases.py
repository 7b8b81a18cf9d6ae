"""Case builders of the sparse and low-rank uplink tests (tests/test_gpu_sparse.py, tests/test_gpu_lowrank.py and the host
files beside them): CPU data only, checked against independent evaluations by tests/test_uplink_cases.py.  A plain module, no tests."""
import numpy as np
import torch

import lowrank_ref
import sparse_ref
from flame_amd import lowrank, sparse

# ---------------------------------------------------------------------------------------------- sparse: the arithmetic case
SUB = 1024
NUMELS = {"a": 1, "b": 1023, "c": 1024, "d": 1025, "e": 4097, "f": 3 * 4096 + 5}
COUNTS = (0, 1, 64, 65, 1024)      # entries per (client, sub-range): none, one, a full step, a step and one, dense
SPARE, HIT = 5, 7                   # element 5 of every key is never sent; every client sends element 7 of e and f


def sparse_case(n, numels=NUMELS):        # (base, updates): updates[c][key] = (int32 indices, fp32 values), numpy
    rng = np.random.default_rng(n)
    base = {k: rng.standard_normal(m).astype(np.float32) for k, m in numels.items()}
    mags = np.float32(10.0) ** rng.permutation(np.linspace(-30, 30, n)).astype(np.float32)     # a wrong order changes bits
    ups = []
    for c in range(n):
        up, empty = {}, n >= 8 and c == 3                       # a client with nnz == 0
        for ki, (k, m) in enumerate(numels.items()):
            idx = [HIT] if k in "ef" and not empty else []
            for s in range(-(-m // SUB)):
                lo, hi = s * SUB, min(m, (s + 1) * SUB)         # (sub-range 0 stays under 66 entries: SPARE is untouched)
                cnt = 0 if empty else min(COUNTS[(c + s + ki) % 5], hi - lo, 65 if s == 0 else SUB)
                edges = [lo, hi - 1] if cnt >= 2 else [hi - 1 if c % 2 else lo][:cnt]
                pool = np.setdiff1d(np.arange(lo, hi), edges + [SPARE, HIT])
                idx += edges + rng.choice(pool, max(0, min(cnt - len(edges), pool.size)), replace=False).tolist()
            idx = np.unique(np.asarray(idx, dtype=np.int32))
            val = (rng.standard_normal(idx.size) * 1e-2).astype(np.float32)
            val[idx == HIT] = mags[c] * (-1) ** c if k in "ef" else val[idx == HIT]
            if k == "d" and idx.size >= 3:
                val[:3] = (1.5e-38, np.inf, np.nan)             # a subnormal product, inf, NaN
            up[k] = (idx, val)
        ups.append(up)
    for k, m in numels.items():
        base[k][SPARE:SPARE + 1] = -0.0
    if "d" in numels:
        base["d"][ups[0]["d"][0][0]] = 0.0                      # the subnormal product lands on a zero and stays
    return base, ups


def rates_of(n):
    return [(c + 1) / (n * (n + 1) / 2) for c in range(n)]


def sparse_weights(up, numels, place=lambda a: torch.from_numpy(a.copy())):
    """One client of :func:`sparse_case` as a SparseWeights; ``place(numpy array) -> tensor`` puts a tensor where the test wants it."""
    return sparse.SparseWeights({k: place(v) for k, (_, v) in up.items()}, {k: place(i) for k, (i, _) in up.items()},
                                {k: (numels[k],) for k in up})


def sparse_want(base, ups, rates, keys=None):
    """``{key: fp32 tensor}`` by tests/sparse_ref.py: key ``k`` after the updates that carry it, in order, each at its own rate."""
    return {k: torch.from_numpy(sparse_ref.accumulate(np.asarray(base[k]), [u[k] for u in ups if k in u], [r for u, r in zip(ups, rates) if k in u]))
            for k in (keys or base)}


# ---------------------------------------------------------------------------------------------- sparse: ragged key sets
GROUP_NUMELS = {"w": 4099, "v": 1025, "b": 77}
V_CARRIERS = (1, 3, 4)
GROUP_RATES = [0.25, 0.125, 0.3, 0.0625, 0.2, 0.0625]


def sparse_group_case(bad=False):
    """``(model, ups)``: model ``{"w": 4099, "v": 1025, "b": 77, "n": int64 0-dim}`` (CPU tensors) and 6 SparseWeights.  All six hold
    ``w`` sparse, ``b`` dense and ``n``; only updates 1, 3 and 4 hold ``v`` (sparse): two client groups.  ``bad``: update 3's ``v``
    repeats its second index at its third position -- ONE bad entry, in the update at entry position 3, in-group position 1."""
    g = torch.Generator().manual_seed(77)
    model = {k: torch.randn(m, generator=g) for k, m in GROUP_NUMELS.items()}
    model["n"] = torch.tensor(3)
    ups = []
    for c in range(6):
        dense = {k: torch.randn(v.shape, generator=g) * 0.01 if v.is_floating_point() else torch.tensor(10 + c) for k, v in model.items()
                 if k != "v" or c in V_CARRIERS}
        w = sparse.topk({k: dense[k] for k in dense if k in "wv"}, ratio=0.05)
        ups.append(sparse.SparseWeights({k: w[k] if k in w else dense[k] for k in dense}, w.indices, w.shapes))
    if bad:
        i = ups[3].indices["v"].clone()
        i[2] = i[1]
        ups[3].indices["v"] = i
    return model, ups


def as_numpy(ups, keys):       # SparseWeights -> the (indices, values) pairs of sparse_ref, for the sparse keys each one carries
    return [{k: (u.indices[k].numpy(), u[k].numpy()) for k in keys if k in u.indices} for u in ups]


# ---------------------------------------------------------------------------------------------- sparse: validation at width
WIDE = {"p": 3 * 4096 + 5, "q": 1025}          # p: 4 chunks, so 4 position slices per client; 300 entries: 75 per slice
WIDE_NNZ, WIDE_PER = 300, 75
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# client 1, key p: position -> (kind, how the bad index is made from the good array g and the key's numel m)
PLANTED_P = {0: ("INT32_MIN", lambda g, m: I32_MIN), 63: ("duplicate", lambda g, m: g[62]), 64: ("descending", lambda g, m: g[61]),
             74: (">= numel", lambda g, m: m), 75: ("negative", lambda g, m: -1), 299: ("INT32_MAX", lambda g, m: I32_MAX)}
# client 2, key q (40 entries)
PLANTED_Q = {17: ("duplicate", lambda g, m: g[16]), 39: (">= numel", lambda g, m: m + 5)}
SEAMS = ((0, 3000), (3001, 4095), (4096, 8191), (8192, 3 * 4096 + 4))     # the value range of each 75-position slice of a good p


def bad_count(idx, numel):
    """flame_sparse_index's stated rule in numpy: an entry is bad when it is negative, or >= numel, or not greater than its predecessor."""
    idx = np.asarray(idx, dtype=np.int64)
    bad = (idx < 0) | (idx >= numel)
    bad[1:] |= idx[1:] <= idx[:-1]
    return int(bad.sum())


def wide_case(bad):
    """``(base, ups)`` as :func:`sparse_case` gives them: 3 clients over ``WIDE``.  Every good ``p`` array has 300 strictly ascending
    entries whose slice j (positions 75 j .. 75 j + 74) starts and ends on ``SEAMS[j]``: positions 74 | 75, 149 | 150 and 224 | 225 hold
    consecutive integers (4095 | 4096 is also the chunk seam), position 0 holds 0 and position 299 the last element.  ``bad``: client
    1's ``p`` gets ``PLANTED_P`` and client 2's ``q`` ``PLANTED_Q``; every other array stays good."""
    rng = np.random.default_rng(5)
    base = {k: rng.standard_normal(m).astype(np.float32) for k, m in WIDE.items()}
    ups = []
    for c in range(3):
        p = np.concatenate([np.sort(np.concatenate([[lo, hi], rng.choice(np.arange(lo + 1, hi), WIDE_PER - 2, replace=False)])) for lo, hi in SEAMS])
        q = np.sort(rng.choice(WIDE["q"], 40, replace=False))
        up = {"p": p.astype(np.int64), "q": q.astype(np.int64)}
        if bad:
            for key, planted in ((("p", PLANTED_P),) if c == 1 else (("q", PLANTED_Q),) if c == 2 else ()):
                good = up[key].copy()
                for pos, (_, make) in planted.items():
                    up[key][pos] = make(good, WIDE[key])
        ups.append({k: (i.astype(np.int32), rng.standard_normal(i.size).astype(np.float32)) for k, i in up.items()})
    return base, ups


# ---------------------------------------------------------------------------------------------- low-rank
LR_SHAPES = {"b": (31, 33), "f": (129, 127), "g": (257, 130)}       # the tile is 128
LR_RANKS = (0, 1, 3, 8, 16)


def lowrank_case(dtype, integer=False, shapes=LR_SHAPES, n=5, carriers=None, seed=0, ranks=None):
    """``(base {k: fp32 numpy [m, n]}, ups[c] = {k: (U, V)} torch CPU factors of dtype[k] or dtype)``: client ``c`` holds key number
    ``ki`` at rank ``LR_RANKS[(c + ki) % 5]`` (rotated per key: every key meets rank 0 and the odd ranks 1 and 3 when n = 5).
    ``carriers``: ``{key: clients that hold it}`` (default: all); ``ranks``: ``{key: one rank per client}`` instead.  Magnitudes in [2^-6, 2^6], or integers of [-8, 8]."""
    rng = np.random.default_rng(4000 + seed + integer)
    draw = (lambda *s: rng.integers(-8, 9, s).astype(np.float32)) if integer else (
        lambda *s: (rng.choice([-1.0, 1.0], s) * 2.0 ** rng.uniform(-6, 6, s)).astype(np.float32))
    dt = dtype if isinstance(dtype, dict) else {k: dtype for k in shapes}
    base = {k: draw(*s) for k, s in shapes.items()}
    ups = []
    for c in range(n):
        up = {}
        for ki, (k, (m, nn)) in enumerate(shapes.items()):
            if carriers is None or c in carriers.get(k, range(n)):
                r = LR_RANKS[(c + ki) % 5] if ranks is None else ranks[k][c]
                up[k] = (torch.from_numpy(draw(m, r)).to(dt[k]), torch.from_numpy(draw(r, nn)).to(dt[k]))
        ups.append(up)
    return base, ups


def lowrank_weights(up, shapes, place=lambda t: t.clone()):
    return lowrank.LowRankWeights({k: place(u) for k, (u, _) in up.items()}, {k: place(v) for k, (_, v) in up.items()}, {k: shapes[k] for k in up})


def lowrank_check(label, got, base, ups, rates, bitwise=False):
    """``got[k]`` (fp32 tensors) against tests/lowrank_ref.py over the clients that carry ``k``: all finite, and every element
    within gamma_{K+1} * mag of the fp64 sum (K = sum r_c); ``bitwise``: the fp32 rounding of the (exact) sum."""
    for k in base:
        held = [(tuple(f.float().numpy() for f in up[k]), r) for up, r in zip(ups, rates) if k in up]
        exact, mag = lowrank_ref.accumulate(base[k], [f for f, _ in held], [r for _, r in held])
        got64 = got[k].detach().cpu().numpy().astype(np.float64).reshape(exact.shape)
        assert np.isfinite(exact).all() and np.isfinite(got64).all(), f"{label}/{k}: a non-finite element"
        err, tol = np.abs(got64 - exact), lowrank_ref.gamma(sum(u.shape[1] for (u, _), _ in held) + 1) * mag
        assert (err <= tol).all(), f"{label}/{k}: {int((err > tol).sum())} elements outside the bound, worst {np.max(err / np.maximum(tol, 1e-300)):.3g} of it"
        if bitwise:
            assert np.array_equal(got64.astype(np.float32).view(np.int32), exact.astype(np.float32).view(np.int32)), f"{label}/{k}: bits differ"


POW2_RATES = [0.5, 0.25, 0.125, 0.0625, 0.0625]


# ---------------------------------------------------------------------------------------------- residency
def place(t, where, device="cuda:0"):
    """A copy of ``t`` (a numpy array or a CPU tensor) on ``where``: "gpu", "pinned", or pageable host memory (anything else)."""
    t = torch.from_numpy(t.copy()) if isinstance(t, np.ndarray) else t.clone()
    return t.to(device) if where == "gpu" else t.pin_memory() if where == "pinned" else t


def _bytes(t):
    flat = t.detach().cpu().contiguous().reshape(-1)
    return flat.view(torch.uint8).clone() if flat.numel() else torch.empty(0, dtype=torch.uint8)     # (an empty tensor has no unit stride to view)


def snapshot(tensors):
    """What a call must leave alone of tensors it only reads: the bytes, the device, the pinning, shape and strides."""
    return [(t, _bytes(t), t.device, tuple(t.shape), t.stride(), (not t.is_cuda) and t.is_pinned()) for t in tensors]


def assert_unchanged(label, snap, bytes_too=True):
    for i, (t, b, dev, shape, stride, pinned) in enumerate(snap):
        assert t.device == dev and tuple(t.shape) == shape and t.stride() == stride, f"{label}: tensor {i} moved or was reshaped"
        assert ((not t.is_cuda) and t.is_pinned()) == pinned, f"{label}: tensor {i}: pinning changed"
        assert not bytes_too or torch.equal(_bytes(t), b), f"{label}: tensor {i} was written"
