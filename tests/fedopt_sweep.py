"""Operand injection for the FedOPT step sweeps (tests/test_gpu_fedopt_sweep16.py,
tests/test_gpu_fedopt_sweep32.py, tests/test_fedopt_sweep_ref.py).

One adaptive step whose root and quotient operands are exactly the injected tensors: with
beta_1 = 1, eta = 1 (FedAdam: beta_2 = 1), current = 0 and one client whose count is the round's
total and whose update is 0, the round's average equals current, d = 0, so m' = m, v' = v,
num = m in all three variants and current' = RN(0 + RN(m / RN(RN(sqrt(v)) + tau))): the output
carries the quotient's own bits.  The same injection runs on the library's optimizer (the per-call
fused launch or the deferred eager chain) and on OracleFedOPT.

A sweep is a set of SOURCE operand vectors (m, v, the client's update) with two extra entries, a
poison element (v = +inf: its lane takes the general sequences) and a pad element (ordinary).  A
packing is an index map from tensor positions to source entries, so that the same sweep can be
laid out with every lane pure, every lane poisoned, or every other lane poisoned; the step is
elementwise, so the oracle runs once on the source and its results go through the same map.
"""
from collections import OrderedDict
import functools

import numpy as np
import torch

import scenarios as S

SORTS = ["fedadam", "fedyogi", "fedadagrad"]
PACKINGS = ["pure", "poisoned", "alternating"]
LAYOUTS = ["aligned", "misaligned"]
KERNELS = ["fused", "chain"]
LANE = {torch.bfloat16: 8, torch.float16: 8, torch.float32: 4, torch.float64: 2}   # elements per lane vector
INT = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32,
       torch.float64: torch.int64}
NP_UINT = {torch.bfloat16: np.uint16, torch.float16: np.uint16, torch.float32: np.uint32, torch.float64: np.uint64}
MANT_BITS = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23, torch.float64: 52}
EXP_BIAS = {torch.bfloat16: 127, torch.float16: 15, torch.float32: 127, torch.float64: 1023}
MAX_ELEMS = {torch.bfloat16: 1 << 23, torch.float16: 1 << 23, torch.float32: 1 << 22,
             torch.float64: 1 << 21}    # 16 MB per tensor
M_ORDINARY = 1.4140625          # exact in every dtype here (1 + 53/128)


def from_bits(bits, dtype):
    """A tensor of ``dtype`` with the given bit patterns (any integer sequence / array)."""
    a = np.asarray(bits, dtype=np.uint64).astype(NP_UINT[dtype])
    return torch.from_numpy(a.view(a.dtype.name[1:])).view(dtype)


def all_patterns16(dtype):
    return from_bits(np.arange(1 << 16), dtype)


def collapse_hyper(sort, tau):
    """The hyperparameters under which one step leaves m and v as injected and num = m."""
    h = {"beta_1": 1.0, "eta": 1.0, "tau": tau}
    if sort == "fedadam":
        h["beta_2"] = 1.0
    return h


# ------------------------------------------------------------------ operand lists
def binade_values(dtype, top_bits, count, seed):
    """Bit patterns of ``count`` non-negative values: +0, the smallest and the largest subnormal,
    and at least one value in every binade of normals up to ``top_bits`` (the largest admitted v),
    with mantissas 0, all-ones and a seeded random one: each binade gets one of the three kinds in
    turn, then -- while a whole pass fits and leaves 16 values -- the other two kinds.  The rest
    are squares of short roots, (9/8 .. 15/8)^2 x 4^k with k spread over the range: their roots are
    exact and have 4 significant bits, and a quotient can be an exact rounding midpoint only over a
    den with a short significand (num = (2q + 1) x den / 2 has to fit the dtype), which is where a
    quotient built from an approximate reciprocal is most likely to round the other way."""
    mb = MANT_BITS[dtype]
    ones = (1 << mb) - 1
    rng = np.random.RandomState(seed)
    e_top = top_bits >> mb
    assert 3 + e_top <= count, (e_top, count)
    out, seen = [], set()

    def take(b):
        if 0 <= b <= top_bits and b not in seen and len(out) < count:
            seen.add(b)
            out.append(b)

    for b in (0, 1, ones):
        take(b)

    def mant(kind):
        return 0 if kind == 0 else ones if kind == 1 else int(rng.randint(1, ones))

    for k in range(3):
        if k and count - len(out) - e_top < 16:
            break
        for e in range(1, e_top + 1):
            b = (e << mb) | mant((e + k) % 3)
            take(b if b <= top_bits else e << mb)
    assert len(out) >= 3 + e_top
    spare = count - len(out)
    bias = EXP_BIAS[dtype]
    k_lo, k_hi = -((bias - 1) // 2), (e_top - bias - 2) // 2        # 2^(1 - bias) <= 4^k and 4 x 4^k <= 2^(e_top - bias)
    for i in range(spare):
        j = 1 + i % 7
        k = k_lo + (i * (k_hi - k_lo)) // max(1, spare - 1)
        v = torch.tensor(((8 + j) / 8.0) ** 2 * 4.0 ** k, dtype=torch.float64).to(dtype)
        assert float(v) == ((8 + j) / 8.0) ** 2 * 4.0 ** k              # exact in the dtype
        take(int(v.view(INT[dtype])))
    while len(out) < count:                             # (duplicates above: random mantissas)
        take((int(rng.randint(1, e_top + 1)) << mb) | mant(2))
    return out


V_TOP = {torch.bfloat16: 0x6680, torch.float16: 0x7BFF, torch.float32: 0x66800000}    # 2^78, 65504, 2^78
V_COUNT = {torch.bfloat16: 224, torch.float16: 128, torch.float32: 256}


def quotient_v_bits(dtype):
    return binade_values(dtype, V_TOP[dtype], V_COUNT[dtype], seed=20 + MANT_BITS[dtype])


def grid_bits(dtype, exponents, seed):
    """exponent fields x mantissas {0, 1, the top bit, all-ones, 12 seeded random}, non-negative."""
    mb = MANT_BITS[dtype]
    rng = np.random.RandomState(seed)
    half = mb // 2
    rand = [(int(rng.randint(0, 1 << half)) << (mb - half)) | int(rng.randint(0, 1 << (mb - half))) for _ in range(12)]
    mants = [0, 1, 1 << (mb - 1), (1 << mb) - 1] + rand
    return [(e << mb) | m for e in exponents for m in mants]


class Source:
    """A sweep's operands: n sweep entries, then the poison entry (index n), then the pad entry."""

    def __init__(self, dtype, m, v, client=None):
        n = m.numel()
        assert v.numel() == n and m.dtype == v.dtype == dtype
        client = torch.zeros(n, dtype=dtype) if client is None else client
        tail = lambda a, b: torch.tensor([a, b], dtype=dtype)
        self.dtype, self.n = dtype, n
        self.m = torch.cat([m, tail(M_ORDINARY, M_ORDINARY)])
        self.v = torch.cat([v, tail(float("inf"), 1.0)])
        self.client = torch.cat([client, tail(0.0, 0.0)])
        self._dev, self._pieces = None, {}

    def pieces(self, per_piece):
        """The sweep cut into sources of at most ``per_piece`` sweep entries (one launch each)."""
        if self.n <= per_piece:
            return [(0, self)]
        if per_piece not in self._pieces:
            cut = lambda t, a: t[a:min(a + per_piece, self.n)]
            self._pieces[per_piece] = [(a, Source(self.dtype, cut(self.m, a), cut(self.v, a), cut(self.client, a)))
                                       for a in range(0, self.n, per_piece)]
        return self._pieces[per_piece]

    def dev(self, device):
        if self._dev is None:
            self._dev = tuple(t.to(device) for t in (self.m, self.v, self.client))
        return self._dev


def root_source(dtype):
    """v = every 16-bit pattern, m = one ordinary value."""
    v = all_patterns16(dtype)
    return Source(dtype, torch.full((1 << 16,), M_ORDINARY, dtype=dtype), v)


def quotient_source(dtype):
    """m = every 16-bit pattern, crossed with quotient_v_bits(dtype): entry vi * 65536 + mi."""
    vb = quotient_v_bits(dtype)
    v = from_bits(vb, dtype).repeat_interleave(1 << 16)
    return Source(dtype, all_patterns16(dtype).repeat(len(vb)), v)


def moment_states(dtype):
    """64 (m, v) states: +-0, the smallest subnormal, the largest finite, +-inf and NaN each as m
    and as v (beside an ordinary partner, and paired with themselves), v's whose v - d^2 is
    exactly 0 for some d, and seeded ordinary values."""
    fi = torch.finfo(dtype)
    sub = float(from_bits([1], dtype)[0])
    special = [0.0, -0.0, sub, fi.max, float("inf"), float("-inf"), float("nan")]
    pairs = [(s, 0.5) for s in special] + [(0.375, s) for s in special] + [(s, s) for s in special]
    pairs += [(0.75, 4.0), (-0.75, 0.25), (3.0, 2.0 ** -14), (-1e-3, 9.0), (0.0, 1.0)]     # d = 2, .5, 2^-7, 3, 1
    g = torch.Generator().manual_seed(64)
    k = 64 - len(pairs)
    mo = torch.randn(k, generator=g) * torch.pow(2.0, torch.randint(-8, 5, (k,), generator=g).float())
    vo = torch.randn(k, generator=g).abs() * torch.pow(2.0, torch.randint(-12, 7, (k,), generator=g).float())
    pairs += list(zip(mo.tolist(), vo.tolist()))
    assert len(pairs) == 64
    return (torch.tensor([p[0] for p in pairs], dtype=torch.float64).to(dtype),
            torch.tensor([p[1] for p in pairs], dtype=torch.float64).to(dtype))


def moment_source(dtype):
    """The client's update d = every 16-bit pattern, crossed with moment_states: entry si * 65536 + di."""
    m, v = moment_states(dtype)
    return Source(dtype, m.repeat_interleave(1 << 16), v.repeat_interleave(1 << 16),
                  all_patterns16(dtype).repeat(m.numel()))


# ------------------------------------------------------------------ packings
def sweep_capacity(packing, lane, length):
    """How many sweep entries ``length`` positions (whole lanes) hold under a packing."""
    groups = length // lane
    if packing == "pure":
        return groups * lane
    if packing == "poisoned":
        return groups * (lane - 1)
    return (groups + 1) // 2 * lane + groups // 2 * (lane - 1)


@functools.lru_cache(maxsize=8)
def pack_index(n, packing, lane, chunk):
    """(src, is_sweep): for each position of the packed tensor the source entry it holds, and
    whether that is a sweep entry.  Lanes are the aligned groups of ``lane`` positions.  pure:
    sweep entries only; poisoned: one slot of every lane (a different one from lane to lane) holds
    the poison entry; alternating: every other lane does.  The tail is padded with the pad entry
    to whole chunks."""
    length = -(-n // (lane - 1)) * lane + lane
    pos = torch.arange(length)
    g, s = pos // lane, pos % lane
    if packing == "pure":
        poison = torch.zeros(length, dtype=torch.bool)
    elif packing == "poisoned":
        poison = s == g % lane
    else:
        poison = (g % 2 == 1) & (s == (g // 2) % lane)
    rank = torch.cumsum(~poison, 0) - 1
    used = int((~poison & (rank == n - 1)).nonzero()[0]) + 1     # positions up to the last sweep entry
    used = -(-used // lane) * lane
    total = -(-used // chunk) * chunk
    src = torch.where(poison, torch.tensor(n), torch.where(rank < n, rank, torch.tensor(n + 1)))[:used]
    src = torch.cat([src, torch.full((total - used,), n + 1, dtype=torch.int64)])
    is_sweep = src < n
    assert int(is_sweep.sum()) == n
    return src, is_sweep


def chunk_elems(dtype):
    from flame_amd import engine
    return engine.chunk_elems(engine.dtype_code(dtype))


# ------------------------------------------------------------------ one step, both sides
def _cache(update, count):
    c = S.SortedCache()
    c["e000"] = S.TR({"w": update}, count)
    return c


def oracle_step(sort, hyper, cur, m, v, client, sqrt_rn=False):
    """(current', m', v') of one injected step on OracleFedOPT (CPU tensors; the inputs are kept)."""
    from oracle import oracle as O
    ora = O.OracleFedOPT(sort, sqrt_rn=sqrt_rn, **hyper)
    ora.current_weights = OrderedDict(w=cur.clone())
    ora.m_t, ora.v_t = {"w": m.clone()}, {"w": v.clone()}
    out = ora.do({"w": cur.clone()}, _cache(client.clone(), 3), total=3)
    return out["w"], ora.m_t["w"], ora.v_t["w"]


def same_or_both_nan(a, b):
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def oracle_collapsed(sort, tau, src, sqrt_rn=False):
    """The oracle's (current', m', v') on a source under collapse_hyper, after asserting that the
    collapse holds there: m' and v' are the injected tensors but for NaN payloads and -0 + 0."""
    zero = torch.zeros(src.n + 2, dtype=src.dtype)
    assert not src.client.any()
    cur, m, v = oracle_step(sort, collapse_hyper(sort, tau), zero, src.m, src.v, src.client, sqrt_rn=sqrt_rn)
    assert bool(same_or_both_nan(m, src.m).all()), f"{sort}: the oracle's m' is not the injected m"
    assert bool(same_or_both_nan(v, src.v).all()), f"{sort}: the oracle's v' is not the injected v"
    return cur, m, v


def _place(t, layout):
    """aligned: the tensor as allocated (16-byte aligned: the vector path); misaligned: a view one
    element into its buffer (the per-element path)."""
    if layout == "aligned":
        out = t.clone()
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t)
    out = buf[1:]
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def gpu_step(sort, hyper, kernel, layout, cur, m, v, client):
    """(current', m', v') of one injected step on the library's optimizer: the per-call fused launch
    (kernel == "fused") or the deferred eager chain ("chain"); asserts through the launch-branch
    counters that exactly that entry point ran, once, and nothing else."""
    from flame_amd import _native
    from flame_amd.optimizers import optimizer_provider
    opt = optimizer_provider.get(sort, defer=kernel == "chain", **hyper)
    opt.current_weights = OrderedDict(w=_place(cur, layout))
    opt.m_t, opt.v_t = {"w": _place(m, layout)}, {"w": _place(v, layout)}
    base = {"w": _place(cur, layout)}
    before = _native.launch_branch_counts()
    out = opt.do(base, _cache(_place(client, layout), 3), total=3)
    new = dict(out)["w"]            # reading a deferred result runs the queue
    m2, v2 = opt.m_t["w"], opt.v_t["w"]
    torch.cuda.synchronize()
    after = _native.launch_branch_counts()
    hits = {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}
    entry = "flame_fedopt_reduce_adapt" if kernel == "fused" else "flame_fedopt_chain"
    assert sum(hits.values()) == 1 and all(k.startswith(entry) for k in hits), (kernel, hits)
    if kernel == "fused":
        assert not any(k.startswith("flame_fedopt_chain") for k in hits), hits
    return new, m2, v2


def _hex(t, i):
    """Element i's bit pattern."""
    width = t.element_size() * 2
    b = int(t[i:i + 1].cpu().view(INT[t.dtype]).item()) & ((1 << 4 * width) - 1)
    return f"{b:#0{width + 2}x}"


def compare(label, got, exp, operands):
    """NaN positions equal and every other element bitwise equal (the sign of zero included).
    Returns the mask of the elements compared bitwise.  ``operands``: name -> tensor, printed for
    the first mismatches."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, (label, got.dtype, exp.dtype, got.shape, exp.shape)
    nan = torch.isnan(exp)
    differ = got.view(INT[got.dtype]) != exp.view(INT[exp.dtype])
    bad = ((torch.isnan(got) != nan) | (differ & ~nan)).nonzero().flatten()
    if bad.numel():
        first = bad[:6]
        rows = []
        for i in first.tolist():
            ops = ", ".join(f"{k}={float(t[i])!r} ({_hex(t, i)})" for k, t in operands.items())
            rows.append(f"[{i}] {ops}: got {float(got[i])!r} ({_hex(got, i)}) want {float(exp[i])!r} ({_hex(exp, i)})")
        raise AssertionError(f"{label}: {bad.numel()} of {got.numel()} elements differ from the oracle:\n  "
                             + "\n  ".join(rows))
    return ~nan


def run_case(label, sort, hyper, kernel, layout, packing, src, expected, device="cuda:0"):
    """One sweep through one kernel, layout and packing, compared with ``expected`` (the oracle's
    (current', m', v') on the source, see oracle_collapsed / oracle_step).  The source is cut into
    launches of at most 16 MB per tensor.  Returns, per output, the mask over the sweep's entries of
    those compared bitwise."""
    dtype = src.dtype
    lane, chunk = LANE[dtype], chunk_elems(dtype)
    per_piece = sweep_capacity(packing, lane, MAX_ELEMS[dtype] // chunk * chunk)
    masks = {k: torch.zeros(src.n, dtype=torch.bool) for k in ("current", "m", "v")}
    for start, piece in src.pieces(per_piece):
        idx, is_sweep = pack_index(piece.n, packing, lane, chunk if layout == "aligned" else lane)
        assert idx.numel() <= MAX_ELEMS[dtype]
        idx_d = idx.to(device)
        sel = None if piece is src else torch.cat([torch.arange(start, start + piece.n),
                                                   torch.tensor([src.n, src.n + 1])]).to(device)
        m, v, client = (t[idx_d] for t in piece.dev(device))
        cur = torch.zeros_like(m)
        got = gpu_step(sort, hyper, kernel, layout, cur, m, v, client)
        ops = {"v": v, "m": m, "d": client}
        where = f"{label} tau={hyper.get('tau')} {packing}/{layout}/{kernel}"
        for name, g, e in zip(("current", "m", "v"), got, expected):
            e_d = (e.to(device) if sel is None else e.to(device)[sel])[idx_d]
            compared = compare(f"{where}/{name}", g, e_d, ops)
            # a sweep entry sits at exactly one position: scatter the mask back to source order
            keep = is_sweep.to(device)
            part = torch.zeros(piece.n, dtype=torch.bool, device=device)
            part[idx_d[keep]] = compared[keep]
            masks[name][start:start + piece.n] = part.cpu()
    return masks


# ------------------------------------------------------------------ the plain reference (host)
def round_f64_to(x, dtype):
    """float64 -> bf16 / fp16 with ONE round-to-nearest-even: round-to-odd into fp32 (24 bits keep a
    sticky bit below every 16-bit rounding point), then the integer rounding on the bits."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = x.astype(np.float32)
        over = np.abs(f.astype(np.float64)) > np.abs(x)              # rounded away from zero: step back
        b = f.view(np.uint32).copy()
        b[over] -= 1                                                  # toward zero (inf -> the largest finite)
        inexact = b.view(np.float32).astype(np.float64) != x
        inexact &= ~np.isnan(x)
        b[inexact] |= 1                                               # round to odd
    if dtype == torch.float16:
        with np.errstate(all="ignore"):
            return torch.from_numpy(b.view(np.float32).astype(np.float16))
    nan = np.isnan(x)
    r = ((b.astype(np.uint64) + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    r[nan] = 0x7FC0
    return torch.from_numpy(r.view(np.int16)).view(torch.bfloat16)


def plain_reference(m, v, tau, dtype):
    """current' of the collapsed step, every op in float64 and rounded once to the dtype:
    RN(m / RN(RN(sqrt(v)) + RN(tau)))."""
    f64 = lambda t: t.to(torch.float64).numpy()
    with np.errstate(all="ignore"):
        t = f64(round_f64_to(np.float64(tau).reshape(1), dtype))[0]
        s = f64(round_f64_to(np.sqrt(f64(v)), dtype))
        den = f64(round_f64_to(s + t, dtype))
        q = f64(round_f64_to(f64(m) / den, dtype))
        return round_f64_to(0.0 + q, dtype)
