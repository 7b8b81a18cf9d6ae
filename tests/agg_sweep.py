"""Operands, layouts and expectations of the aggregation sweeps (tests/test_gpu_agg_sweep16.py,
tests/test_gpu_agg_sweep_wide.py, tests/test_agg_sweep_ref.py).

The same-dtype aggregation kernels (flame_agg_reduce, flame_agg_reduce_scaled,
flame_fedbuff_scale_add, flame_hier_fedbuff in both modes, flame_feddyn_round) are built from four
small functions of csrc/fedagg.hip: the product ``v * rate`` rounded to the dtype, the sum
``acc + tmp`` rounded to the dtype, the quotient ``a / goal`` (with the delta ``w' - w``) and the
sync hierarchy's ``rnd(w' - w)``.  A 16-bit dtype has 65,536 values, so every one of them goes
through each function in each kernel: as the only operand where the op has one (the product, the
quotient), and crossed with a list of 64 accumulators where it has two (the sum, the quotient + sum,
the delta, FedDyn's history sum).  f32 and f64 have no exhaustive list: their "patterns" are
fedopt_sweep.grid_bits over every exponent field with both signs, crossed with 16 accumulators.

The expectation is never the library's: it is the torch-CPU restatement of the reference's own
statements (uplink16_case.restate, oracle/torch_cpu.py's fedbuff_step / fedbuff_scale_add /
fedavg_round, and the hierarchy / FedDyn sequences restated below).  Those ops are elementwise, so
an expectation is computed once on the SOURCE operands and indexed into each layout:

  * aligned: whole chunks (the vector path) and then a ragged tail of LANE - 1 elements, which the
    per-element bodies (hier_tail, the VEC = false FedDyn body, the reductions' tails) run;
  * misaligned: a view one element into its buffer (FLAME_SEG_UNALIGNED: the per-element path).
"""
import collections
import functools
import math

import numpy as np
import torch

import fedopt_sweep as F
import scenarios as S
import test_gpu_uplink16 as U16
import uplink16_case as U
from oracle import torch_cpu as T

DTYPES16 = {"bf16": torch.bfloat16, "f16": torch.float16}
DTYPES_WIDE = {"f32": torch.float32, "f64": torch.float64}
LAYOUTS = F.LAYOUTS
EXP_BITS = {torch.bfloat16: 8, torch.float16: 5, torch.float32: 8, torch.float64: 11}
RATES = list(U16.RATES) + [0.3713, float(1 / math.sqrt(2)), float(1 / math.sqrt(3))]     # + FedBuff's staleness rates
SCALES = [1.0, 0.5, 1.0 / 3.0, 2.0 ** -14, 1.9990234375]
GOALS = [1, 2, 3, 7, 10, 64, 65, 100, 1000, 2 ** 20, 2 ** 24 + 1]      # the last is no fp32 value
FLOOR = 60000                               # non-NaN expectations in every row of 65,536 patterns


def wide(dtype):
    return dtype in (torch.float32, torch.float64)


def width(dtype):
    return 8 * torch.empty(0, dtype=dtype).element_size()


def sign_bit(dtype):
    return 1 << (width(dtype) - 1)


def inf_bits(dtype):
    return ((1 << EXP_BITS[dtype]) - 1) << F.MANT_BITS[dtype]


def max_bits(dtype):
    return inf_bits(dtype) - 1


def rows(dtype):
    """Accumulators of one pair tensor."""
    return 16 if wide(dtype) else 64


def floor(dtype):
    """The fewest non-NaN expectations a row of patterns may have: 60,000 of 65,536, the same share
    of a grid row."""
    return patterns(dtype).numel() * FLOOR // (1 << 16)


def rate_triple(i):
    """Three of RATES; every rate is the first client's once as i runs over range(len(RATES))."""
    n = len(RATES)
    return [RATES[i % n], RATES[(i + 1) % n], RATES[(i + 3) % n]]


def scale_triple(i):
    n = len(SCALES)
    return [SCALES[i % n], SCALES[(i + 1) % n], SCALES[(i + 2) % n]]


# ------------------------------------------------------------------ operand lists
@functools.lru_cache(maxsize=None)
def pattern_bits(dtype):
    """The swept operand's bit patterns: every 16-bit pattern (entry j = pattern j), or for f32 /
    f64 fedopt_sweep.grid_bits over every exponent field -- mantissas 0, 1, the top bit, all-ones
    and 12 random -- with both signs."""
    if not wide(dtype):
        return np.arange(1 << 16, dtype=np.uint64)
    pos = np.asarray(F.grid_bits(dtype, range(1 << EXP_BITS[dtype]), seed=90 + F.MANT_BITS[dtype]), dtype=np.uint64)
    return np.concatenate([pos, pos | np.uint64(sign_bit(dtype))])


@functools.lru_cache(maxsize=None)
def patterns(dtype):
    return F.from_bits(pattern_bits(dtype), dtype)


@functools.lru_cache(maxsize=None)
def permutation(dtype, k):
    """A seeded permutation of the patterns that moves every pattern inside its sign and exponent
    field (an infinity stays where it is, a NaN goes to a NaN); an odd ``k`` flips the sign as well.
    So a NaN or an overflow sits at the same entries in every client of a launch and the count of
    elements compared bitwise stays the one-operand count, while every entry still pairs values of
    different mantissas -- and, under an odd k, of opposite signs: cancellation."""
    mb = F.MANT_BITS[dtype]
    bits = pattern_bits(dtype).astype(np.int64)
    n = bits.size
    mag = bits & (sign_bit(dtype) - 1)
    key = ((bits >> mb) & ((2 << EXP_BITS[dtype]) - 1)) * 2 + (mag > inf_bits(dtype))
    rng = np.random.RandomState(1600 + 10 * mb + k)
    where = np.lexsort((np.arange(n), key))             # the entries, grouped by key
    order = np.lexsort((rng.rand(n), key))              # the same groups, shuffled inside
    perm = np.empty(n, dtype=np.int64)
    perm[where] = order
    assert (key[perm] == key).all()
    if k % 2:
        ubits = pattern_bits(dtype)
        flipped = ubits[perm] ^ np.uint64(sign_bit(dtype))
        by_bits = np.argsort(ubits)
        perm = by_bits[np.searchsorted(ubits[by_bits], flipped)]
        assert (ubits[perm] == flipped).all()
    return torch.from_numpy(perm)


def client(dtype, k):
    """Client k's tensor: the patterns themselves (k = 0) or permutation k of them."""
    p = patterns(dtype)
    return p if k == 0 else p[permutation(dtype, k)]


@functools.lru_cache(maxsize=None)
def accumulators(dtype):
    """[blocks, rows] accumulators.  Every block holds +-0, the smallest and the largest subnormal,
    +-max and +-inf, then values of fedopt_sweep.binade_values over the whole finite range
    (mantissas 0, all-ones and random), the signs alternating.  fp16's 30 binades of normals fit
    one block of 64.  bf16 has 254, more than 64 values can hold, so its list is five blocks of 64,
    block b taking every fifth value: every binade appears in one of them.  f32 / f64: one block of
    16, eight values spread over the binades.  No NaN: NaN operands come from the patterns."""
    mb = F.MANT_BITS[dtype]
    top, ones, sb, inf = max_bits(dtype), (1 << mb) - 1, sign_bit(dtype), inf_bits(dtype)
    special = [0, sb, 1, ones, top, top | sb, inf, inf | sb]
    per = rows(dtype) - len(special)
    binades = top >> mb
    vals = [b for b in F.binade_values(dtype, top, 3 + binades + 31, seed=70 + mb) if b not in special]
    assert {b >> mb for b in vals} >= set(range(1, binades + 1))
    if wide(dtype):
        vals = [vals[i * (binades - 1) // (per - 1)] for i in range(per)]        # the first pass: one per binade
        blocks = 1
    else:
        blocks = -(-(3 + binades) // per)
        vals = vals[:blocks * per]
        assert len(vals) == blocks * per
    out = []
    for b in range(blocks):
        mine = vals[b::blocks]
        out.append(special + [v | (sb if i % 2 else 0) for i, v in enumerate(mine)])
    acc = torch.stack([F.from_bits(r, dtype) for r in out])
    assert acc.shape == (blocks, rows(dtype)) and not bool(torch.isnan(acc).any())
    return acc


def finite_accumulators(dtype):
    """Block 0's finite values."""
    a = accumulators(dtype)[0]
    return a[torch.isfinite(a)]


def bases(dtype):
    """The uplink test's bases rounded to the dtype, -inf and the dtype's largest value."""
    return [float(torch.tensor(b, dtype=torch.float64).to(dtype)) for b in U16.BASES] + \
        [float("-inf"), torch.finfo(dtype).max]


def pair(dtype, block=0):
    """(acc, pat): accumulator i x pattern j at entry i * len(patterns) + j (16-bit: 64 x 65,536 =
    4,194,304 entries each)."""
    acc = accumulators(dtype)[block]
    return acc.repeat_interleave(patterns(dtype).numel()), patterns(dtype).repeat(rows(dtype))


# ------------------------------------------------------------------ layouts
@functools.lru_cache(maxsize=32)
def layout_index(n, layout, lane, chunk):
    """Source entry of every position of a tensor that carries n source entries.  aligned: the
    entries, padded with entries from the start up to whole chunks, then LANE - 1 more entries
    spread over the source (the ragged tail).  misaligned: the entries themselves."""
    idx = torch.arange(n)
    if layout == "misaligned":
        return idx
    pad = -n % chunk
    tail = (torch.arange(1, lane) * (n // lane) + 37) % n
    return torch.cat([idx, torch.arange(pad) % n, tail])


def index_for(dtype, n, layout):
    lane = F.LANE[dtype] if dtype in F.LANE else 16 // (width(dtype) // 8)         # (the integer dtypes)
    return layout_index(n, layout, lane, F.chunk_elems(dtype))


def place(t, layout, device="cuda:0"):
    """A fresh device tensor of ``t``'s values: as allocated, or one element into its buffer."""
    if layout == "misaligned":
        return U16._off_by_one(t)
    out = t.to(device, copy=True)
    assert out.data_ptr() % 16 == 0
    return out


# ------------------------------------------------------------------ the restated statements (torch-CPU)
def reduce_restated(base, clients, rates, scales=None):
    """flame_agg_reduce / flame_agg_reduce_scaled: ``tmp = v * rate; base += tmp`` per client;
    ``base`` None is the None start (fedbuff.py's first arrival: the aggregate IS the first tmp)."""
    T.consult.note()
    if base is not None:
        return U.restate(base, clients, rates, scales)
    v = clients[0] if scales is None else torch.mul(clients[0], scales[0])
    tmp = v * rates[0]
    tmp = tmp.to(dtype=v.dtype) if tmp.dtype != v.dtype else tmp
    return U.restate(tmp, clients[1:], rates[1:], None if scales is None else scales[1:])


def scale_add_restated(w, a, goal):
    """(w', delta) of ``w += a / goal`` and the middle's ``delta = w' - w`` (common/util.py:152-159)."""
    new = T.fedbuff_scale_add({"w": w.clone()}, {"w": a}, goal)["w"]
    return new, new - w


def hierarchy_restated(mid_w, arrivals, versions, goals, mid_versions, version, top_agg, top_w, top_goal):
    """flame_amd.optimizer.fedbuff.hierarchy_round as the roles issue it, on torch-CPU: per middle the
    None-start FedBuff aggregate of its arrivals, scale_add + delta, the top's FedBuff step on the
    delta; then the top's scale_add.  Returns (new middle weights, deltas, top aggregate, top weights)."""
    new_w, deltas = [], []
    top_agg = None if top_agg is None else {"w": top_agg.clone()}
    for w, arr, vers, goal, mv in zip(mid_w, arrivals, versions, goals, mid_versions):
        agg = None
        for a, v in zip(arr, vers):
            agg = T.fedbuff_step(agg, {"w": a}, version, v)
        nw, d = scale_add_restated(w, agg["w"], goal)
        new_w.append(nw)
        deltas.append(d)
        top_agg = T.fedbuff_step(top_agg, {"w": d}, version, mv)
    top = T.fedbuff_scale_add({"w": top_w.clone()}, top_agg, top_goal)["w"]
    return new_w, deltas, top_agg["w"], top


def sync_hierarchy_restated(mid_w, arrivals, counts, top_w):
    """flame_amd.optimizer.sync_hierarchy.sync_hierarchy_round on torch-CPU: per middle FedAvg from a
    copy of its weights and ``delta = new - old``; the top's FedAvg over the deltas with rate
    total_m / sum.  Returns (new middle weights, deltas, top weights)."""
    new_w, deltas, totals = [], [], []
    for w, arr, cnt in zip(mid_w, arrivals, counts):
        new = T.fedavg_round({"w": w.clone()}, [{"w": a} for a in arr], cnt, sum(cnt))["w"]
        new_w.append(new)
        deltas.append(new - w)
        totals.append(sum(cnt))
    top = T.fedavg_round({"w": top_w.clone()}, [{"w": d} for d in deltas], totals, sum(totals))["w"]
    return new_w, deltas, top


def feddyn_restated(base, hist, arrivals):
    """One FedDyn.do (feddyn.py:96-139) on torch-CPU.  ``hist``: OrderedDict end -> history tensor or
    None, in local_param_dict's order (updated in place); ``arrivals``: [(end, w)] in cache order.
    Returns (average, cld_model)."""
    T.consult.note()
    avg = base.clone()
    rate = 1 / len(arrivals)
    for e, w in arrivals:
        hist[e] = w if hist.get(e) is None else hist[e] + w
        tmp = w * rate
        avg += tmp.to(dtype=w.dtype) if tmp.dtype != w.dtype else tmp
    mean = 0.0
    rate = 1 / len(hist)
    for e in hist:
        if hist[e] is not None:
            mean = mean + rate * hist[e]
    return avg, avg + mean


# ------------------------------------------------------------------ comparison
def check(label, got, exp):
    """scenarios.same_bits on {name: tensor}: every non-NaN element bitwise, the sign of zero
    included; a NaN meets a NaN."""
    S.same_bits(label, got, exp)


def compared_rows(dtype, exp):
    """Per row of patterns: how many expectations are no NaN (those are compared bitwise)."""
    return (~torch.isnan(exp)).view(-1, patterns(dtype).numel()).sum(1)


# ------------------------------------------------------------------ the cases the GPU tests run, as data
# Each builder returns the operands and the expectation on the SOURCE entries (CPU tensors); the
# GPU tests index both by layout, tests/test_agg_sweep_ref.py establishes the floors on them.
def product_launches(dtype):
    """(launch, init_first, clients) of the product sweep: one launch per rate triple, accumulating
    and from a None start, and one of 9 clients (the unrolled loop of 8 and its remainder)."""
    n = len(RATES) if not wide(dtype) else 4
    return [(i, init, 3) for init in (False, True) for i in range(n)] + [(0, False, 9)]


def product_case(dtype, i, init_first, n_clients=3):
    """Clients 0..n-1 under rate_triple(i) (n = 3) or n of RATES from the i-th on, one segment per
    base (one segment from a None start).  -> (clients, rates, [expectation per segment])."""
    cl = [client(dtype, k) for k in range(n_clients)]
    rates = rate_triple(i) if n_clients == 3 else [RATES[(i + k) % len(RATES)] for k in range(n_clients)]
    n = patterns(dtype).numel()
    if init_first:
        return cl, rates, [reduce_restated(None, cl, rates)]
    return cl, rates, [reduce_restated(torch.full((n,), b, dtype=dtype), cl, rates) for b in bases(dtype)]


def scaled_case(dtype, i):
    """round(round(v * scale) * rate): scale_triple(i) under rate_triple(i), one segment per base."""
    cl = [client(dtype, k) for k in range(3)]
    rates, scales = rate_triple(i), scale_triple(i)
    n = patterns(dtype).numel()
    return cl, rates, scales, [reduce_restated(torch.full((n,), b, dtype=dtype), cl, rates, scales)
                               for b in bases(dtype)]


PAIR_SCALED = (1.0 / 3.0, 0.75)             # the pair launch of the scaled reduction: (scale, rate)


def sum_case(dtype, block):
    """One client at rate 1.0 over a pair tensor: tmp = v exactly, the launch is ``acc + v``."""
    acc, pat = pair(dtype, block)
    return acc, pat, reduce_restated(acc, [pat], [1.0])


def scaled_pair_case(dtype):
    acc, pat = pair(dtype)
    return acc, pat, reduce_restated(acc, [pat], [PAIR_SCALED[1]], [PAIR_SCALED[0]])


def scale_add_block(dtype, goal):
    """The accumulator block goal number g runs against: the blocks in turn."""
    return GOALS.index(goal) % accumulators(dtype).shape[0]


def scale_add_case(dtype, goal):
    """w = the accumulators, a = the patterns.  -> (w, a, w', delta)."""
    w, a = pair(dtype, scale_add_block(dtype, goal))
    new, delta = scale_add_restated(w, a, goal)
    return w, a, new, delta


def finite_rows(dtype, block=0):
    """The rows of a pair tensor whose accumulator is finite (a delta over an infinite one is NaN
    everywhere: inf - inf)."""
    return torch.isfinite(accumulators(dtype)[block])


# ------------------------------------------------------------------ hierarchy shapes
HIER_C = 2
HIER_SEGS = 5
HIER_VERSION = 40
STALE = 35                                  # rate 1 / sqrt(36) = 1/6, see hier_operands
HIER_MIDS = {"reg": 2, "lds": 16}           # register store groups; LDS store groups (>= 16 middles)
INF_MID = (HIER_SEGS - 1, 1)                # (segment, middle) whose weight is +inf
BARE_SEG = HIER_SEGS - 2                    # the segment of -0 weights (see hier_operands)


def hier_operands(dtype, M):
    """Per segment s and middle m a constant middle weight from the accumulator list (finite ones,
    but INF_MID's: +inf, whose delta is NaN everywhere), C = 2 arrivals per middle (middle 0's first
    one carries the patterns, the others permutations; the same tensors for every segment), FedBuff
    versions of staleness 0 / 1 / 2 and 35, goals 3 and 65, sync counts that give rates 1/3 and 2/3 under
    totals of 3 and 6 (so the top's rates are no powers of two either), and the top's weights
    (accumulators) and existing aggregate (a permutation).

    Segment BARE_SEG lets single ops through to an output: every weight in it is -0 and every
    middle's second arrival is -0 (x + -0 = x for every x), so a FedBuff middle's aggregate is its
    first arrival's product and its delta that product's quotient, a sync middle's new weights ARE
    the product, and the top holds the plain sum of the deltas' products."""
    fin = finite_accumulators(dtype)
    n = patterns(dtype).numel()
    nz = torch.full((n,), -0.0, dtype=dtype)
    swept = [[client(dtype, m * HIER_C + t) for t in range(HIER_C)] for m in range(M)]
    arrivals, mid_w, top_w = [], [], []
    for s in range(HIER_SEGS):
        if s == BARE_SEG:
            arrivals.append([[row[0]] + [nz] * (HIER_C - 1) for row in swept])
            mid_w.append([nz] * M)
            top_w.append(nz)
            continue
        # one sign per segment: a middle whose w + x overflows does so toward its weight's sign, so the
        # deltas of a segment never hold both infinities and the top's sum stays a number
        row = [math.copysign(float(fin[(3 + s * M + m) % fin.numel()]), -s % 2 - 0.5) for m in range(M)]
        if s == INF_MID[0]:
            row[INF_MID[1]] = float("inf")
        arrivals.append(swept)
        mid_w.append([torch.full((n,), x, dtype=dtype) for x in row])
        top_w.append(torch.full((n,), float(fin[(5 + 7 * s) % fin.numel()]), dtype=dtype))
    versions = [[HIER_VERSION - (m + t) % 3 for t in range(HIER_C)] for m in range(M)]
    mid_versions = [HIER_VERSION - m % 2 for m in range(M)]
    # the staleness rates 1, 1/sqrt(2), 1/sqrt(3) happen to give the same bits on every 16-bit value
    # whether their product is rounded once or twice; 1/6 does not (tests/test_agg_sweep_ref.py), so
    # the patterns' arrival and middle 1's delta carry it
    versions[0][0] = mid_versions[1] = HIER_VERSION - STALE
    goals = [3 if m % 2 == 0 else 65 for m in range(M)]
    counts = [[1, 2] if m % 2 == 0 else [4, 2] for m in range(M)]
    top_agg = [client(dtype, 40 + 2 * s) for s in range(HIER_SEGS)]
    return dict(mid_w=mid_w, arrivals=arrivals, versions=versions, mid_versions=mid_versions, goals=goals,
                counts=counts, top_w=top_w, top_agg=top_agg, top_goal=M)


def hier_expected(dtype, M, sync, from_none=True):
    """(operands, {name: [per segment]}) of one hierarchy case on the source entries; mid_w and
    delta hold one list per segment with one tensor per middle."""
    o = hier_operands(dtype, M)
    out = collections.defaultdict(list)
    for s in range(HIER_SEGS):
        if sync:
            nw, d, top = sync_hierarchy_restated(o["mid_w"][s], o["arrivals"][s], o["counts"], o["top_w"][s])
        else:
            nw, d, agg, top = hierarchy_restated(o["mid_w"][s], o["arrivals"][s], o["versions"], o["goals"],
                                                 o["mid_versions"], HIER_VERSION,
                                                 None if from_none else o["top_agg"][s], o["top_w"][s], o["top_goal"])
            out["top_agg"].append(agg)
        out["mid_w"].append(nw)
        out["delta"].append(d)
        out["top_w"].append(top)
    return o, dict(out)


# ------------------------------------------------------------------ FedDyn rounds
# local_param_dict's order.  p, q and r are active ends that never arrive: they have no history, but
# count in the mean's rate, 1/6 -- a rate whose product shows whether it was rounded once or twice
# (1/2 and 1/3, the averages' rates here, do not: tests/test_agg_sweep_ref.py)
DYN_ORDERS = {"arrival": ["a", "b", "z", "p", "q", "r"], "shuffled": ["b", "p", "z", "a", "q", "r"]}
DYN_KEYS = ["pair", "zero", "bare"]


def feddyn_operands(dtype):
    """Two rounds.  Round 1: ends a, b and z arrive (their first histories are their w: a's is the
    accumulators, z's is -0 everywhere).  Round 2: a and b arrive -- a's w is the patterns, so
    ``h + w`` is the pair sum -- and z is the HIN | MEAN-only end.  Key "zero" is -0 everywhere in
    every tensor: its mean must come out +0 (``0.0 + sum``), so cld = -0 + +0 = +0 over a -0 average.
    Key "bare" is -0 as well, but for a's round-1 w, the patterns: its average is the bare product
    ``RN(w / 3)`` and its cld that product's double (``x + -0 = x``)."""
    acc, pat = pair(dtype)
    n, n0 = acc.numel(), patterns(dtype).numel()
    r = rows(dtype)
    nz = lambda k: torch.full((k,), -0.0, dtype=dtype)
    z = nz(n0)
    round1 = {"a": {"pair": acc, "zero": z, "bare": patterns(dtype)},
              "b": {"pair": client(dtype, 1).repeat(r), "zero": z, "bare": z},
              "z": {"pair": nz(n), "zero": z, "bare": z}}
    round2 = {"a": {"pair": pat, "zero": z, "bare": z}, "b": {"pair": client(dtype, 2).repeat(r), "zero": z, "bare": z}}
    base = {"pair": torch.full((n,), 0.5, dtype=dtype), "zero": z, "bare": z}
    return base, round1, round2


def feddyn_expected(dtype, order):
    """(operands, [round 1, round 2]); a round is {"avg", "cld", "hist": {end: tensor}} per key.
    Round 2 starts from round 1's cld_model, as the role does."""
    base, round1, round2 = feddyn_operands(dtype)
    rounds = [{}, {}]
    for k in DYN_KEYS:
        hist = collections.OrderedDict((e, None) for e in DYN_ORDERS[order])
        b = base[k]
        for r, arr in enumerate((round1, round2)):
            avg, cld = feddyn_restated(b, hist, [(e, arr[e][k]) for e in sorted(arr)])
            rounds[r][k] = {"avg": avg, "cld": cld, "hist": dict(hist)}
            b = cld
    return (base, round1, round2), rounds


# ------------------------------------------------------------------ integer operands (flame_agg_reduce only)
INT_RATES = [1.0, 1.0 / 3.0, 0.75, 1e-3, -0.5]
INT_TOP = {torch.int32: 30, torch.int64: 62}


def int_values(dtype):
    """+-2^k and +-(2^k +- 1) for k up to 30 (i32) / 62 (i64): beyond 2^24 the int -> fp32
    conversion rounds, and negative products truncate toward zero."""
    v = sorted({s * (2 ** k + d) for k in range(INT_TOP[dtype] + 1) for d in (-1, 0, 1) for s in (1, -1)})
    return torch.tensor(v, dtype=dtype)


def int_case(dtype):
    """(v, bases, rates, keep, expectation per rate): ``tmp = (v * rate).to(int); base += tmp`` per
    value x rate, one client.  ``keep[r]``: the values whose fp32 product with rate r fits the
    integer type -- outside that the reference's cast is undefined behaviour."""
    v = int_values(dtype)
    g = torch.Generator().manual_seed(170 + INT_TOP[dtype])
    info = torch.iinfo(dtype)
    base = torch.randint(info.min // 2, info.max // 2, (v.numel(),), generator=g, dtype=torch.int64).to(dtype)
    base[::3] = info.max - 1            # the wrapping add
    base[1::7] = info.min
    keep, exp = [], []
    for r in INT_RATES:
        p = (v.to(torch.float32) * torch.tensor(r, dtype=torch.float32)).double()
        keep.append((p > float(info.min)) & (p < float(info.max)))
        exp.append(reduce_restated(base, [v], [r]))
    return v, base, INT_RATES, keep, exp


# ------------------------------------------------------------------ the GPU side
DEV = "cuda:0"
_CACHE = collections.OrderedDict()


def cached(key, build):
    """``build()`` once per key; the two most recent keys are kept (the cases are ordered so that
    the key changes last: the layouts and entry points of one case share an expectation)."""
    T.consult.note()        # every case compares with torch-CPU's results, whichever case computed them
    if key not in _CACHE:
        while len(_CACHE) >= 2:
            _CACHE.popitem(last=False)
        _CACHE[key] = build()
    _CACHE.move_to_end(key)
    return _CACHE[key]


class Pinned:
    """The native launches made inside the block: their names (engine._recorders, as
    test_gpu_uplink16.Launches) and the launch branches they took (the C ABI's counters)."""

    def __enter__(self):
        from flame_amd import _native
        self._ln = U16.Launches()
        self._ln.__enter__()
        self._before = _native.launch_branch_counts()
        return self

    def __exit__(self, *exc):
        from flame_amd import _native
        torch.cuda.synchronize()
        self._ln.__exit__(*exc)
        after = _native.launch_branch_counts()
        self.names = self._ln.names
        self.branches = {k: after[k] - self._before.get(k, 0) for k in after if after[k] != self._before.get(k, 0)}
        return False

    def only(self, name, count=1, branch=None):
        """Exactly ``count`` launches, all of entry point ``name`` (and of launch branches that
        start with ``branch``): a case that fell back to a torch path or to separate launches fails."""
        assert self.names == [name] * count, self.names
        if branch is False:         # (flame_agg_reduce_scaled has no launch-branch counter)
            assert not self.branches, self.branches
            return
        assert sum(self.branches.values()) == count, self.branches
        assert all(k.startswith(branch or name) for k in self.branches), (branch or name, self.branches)


def report(label, dtype, counts, keep=None):
    """Print and return the fewest elements compared bitwise in a row of patterns."""
    n = patterns(dtype).numel()
    rows_ = torch.cat([c.flatten() for c in counts])
    least = int((rows_ if keep is None else rows_[keep]).min())
    total = f", {int(rows_.sum())} of {rows_.numel() * n} in all" if rows_.numel() > 1 else ""
    print(f"{label}: compared {least} of {n} per row at least{total}")
    return least


def run_reduce(label, dtype, layout, seg_bases, clients, rates, expected, *, init_first=False, scales=None):
    """One flame_agg_reduce (with ``scales``: flame_agg_reduce_scaled) launch: a segment per entry of
    ``seg_bases`` (source-order CPU tensors; one segment from a None start), the same clients in each."""
    from flame_amd import engine
    idx = index_for(dtype, clients[0].numel(), layout)
    dev_cl = [place(c[idx], layout) for c in clients]
    if init_first:
        outs = [place(torch.full((idx.numel(),), 7, dtype=dtype), layout)]
    else:
        outs = [place(b[idx], layout) for b in seg_bases]
    with Pinned() as pin:
        engine.reduce_(outs, None if init_first else outs, [dev_cl] * len(outs), rates, init_first=init_first,
                       scales=scales)
    if scales is not None:
        pin.only("flame_agg_reduce_scaled", branch=False)
    else:
        pin.only("flame_agg_reduce")
    assert len(outs) == len(expected)
    check(label, {f"seg{j}": o for j, o in enumerate(outs)}, {f"seg{j}": e[idx] for j, e in enumerate(expected)})
    return [compared_rows(dtype, e) for e in expected] if dtype.is_floating_point else None


def run_scale_add(label, dtype, layout, w, a, goal, new, delta, with_delta):
    from flame_amd import engine
    idx = index_for(dtype, w.numel(), layout)
    wd, ad = place(w[idx], layout), place(a[idx], layout)
    dd = place(torch.full((idx.numel(),), 7, dtype=dtype), layout) if with_delta else None
    with Pinned() as pin:
        engine.scale_add_([wd], [ad], goal, [dd] if with_delta else None)
    pin.only("flame_fedbuff_scale_add")
    got, exp = {"w": wd}, {"w": new[idx]}
    if with_delta:
        got["delta"], exp["delta"] = dd, delta[idx]
    check(label, got, exp)
    return compared_rows(dtype, new), compared_rows(dtype, delta)


def _hier_check(label, dtype, idx, exp, mids_w, deltas, top_w, top_agg=None):
    got, want = {}, {}
    for s in range(HIER_SEGS):
        for m in range(len(mids_w)):
            got[f"s{s}/m{m}/w"], want[f"s{s}/m{m}/w"] = mids_w[m][f"s{s}"], exp["mid_w"][s][m][idx]
            got[f"s{s}/m{m}/delta"], want[f"s{s}/m{m}/delta"] = deltas[m][f"s{s}"], exp["delta"][s][m][idx]
        got[f"s{s}/top_w"], want[f"s{s}/top_w"] = top_w[f"s{s}"], exp["top_w"][s][idx]
        if top_agg is not None:
            got[f"s{s}/top_agg"], want[f"s{s}/top_agg"] = top_agg[f"s{s}"], exp["top_agg"][s][idx]
    check(label, got, want)
    counts = {}
    for s in range(HIER_SEGS - 1):          # (the last segment holds the +inf middle: NaN deltas, a NaN top)
        for nm in ("mid_w", "delta"):
            counts.setdefault(nm, []).extend(compared_rows(dtype, e) for e in exp[nm][s])
        for nm in ("top_w", "top_agg"):
            if nm in exp:
                counts.setdefault(nm, []).append(compared_rows(dtype, exp[nm][s]))
    return counts


def _hier_arrivals(o, idx, layout):
    """[segment][middle][arrival] device tensors; a source tensor that several segments share is placed once."""
    placed = {}

    def dev(t):
        if id(t) not in placed:
            placed[id(t)] = place(t[idx], layout)
        return placed[id(t)]
    return [[[dev(a) for a in row] for row in seg] for seg in o["arrivals"]]


def run_hierarchy(label, dtype, layout, M, from_none, o, exp):
    """One flame_hier_fedbuff launch in FedBuff mode through FedBuff.do_arrivals + hierarchy_round:
    middle weights, deltas, top aggregate and top weights."""
    from flame_amd.optimizer.fedbuff import hierarchy_round
    from flame_amd.optimizers import optimizer_provider
    idx = index_for(dtype, patterns(dtype).numel(), layout)
    keys = [f"s{s}" for s in range(HIER_SEGS)]
    arr = _hier_arrivals(o, idx, layout)
    mids_w, middles = [], []
    for m in range(M):
        agg = optimizer_provider.get("fedbuff").do_arrivals(
            None, [S.TR({k: arr[s][m][t] for s, k in enumerate(keys)}, 1, o["versions"][m][t]) for t in range(HIER_C)],
            version=HIER_VERSION)
        mids_w.append({k: place(o["mid_w"][s][m][idx], layout) for s, k in enumerate(keys)})
        middles.append((mids_w[m], agg, o["goals"][m], o["mid_versions"][m]))
    top_w = {k: place(o["top_w"][s][idx], layout) for s, k in enumerate(keys)}
    top_agg = None if from_none else {k: place(o["top_agg"][s][idx], layout) for s, k in enumerate(keys)}
    with Pinned() as pin:
        res, deltas = hierarchy_round(middles, top_agg, version=HIER_VERSION, top_weights=top_w,
                                      top_goal=o["top_goal"], with_delta=True)
    pin.only("flame_hier_fedbuff")
    assert all(("/lds" in k) == (M >= HIER_MIDS["lds"]) and k.endswith("/fedbuff") for k in pin.branches), pin.branches
    return _hier_check(label, dtype, idx, exp, mids_w, deltas, top_w, dict(res))


def run_sync_hierarchy(label, dtype, layout, M, o, exp):
    """The same shapes through sync_hierarchy_round (FLAME_HIER_SYNC): the delta is rnd(w' - w)."""
    from flame_amd.optimizer.sync_hierarchy import sync_hierarchy_round
    idx = index_for(dtype, patterns(dtype).numel(), layout)
    keys = [f"s{s}" for s in range(HIER_SEGS)]
    arr = _hier_arrivals(o, idx, layout)
    mids_w, specs = [], []
    for m in range(M):
        cache = S.SortedCache()
        for t in range(HIER_C):
            cache[f"e{t}"] = S.TR({k: arr[s][m][t] for s, k in enumerate(keys)}, o["counts"][m][t])
        mids_w.append({k: place(o["mid_w"][s][m][idx], layout) for s, k in enumerate(keys)})
        specs.append((mids_w[m], cache, sum(o["counts"][m])))
    top_w = {k: place(o["top_w"][s][idx], layout) for s, k in enumerate(keys)}
    with Pinned() as pin:
        top, deltas = sync_hierarchy_round(specs, top_w, with_delta=True)
    pin.only("flame_hier_fedbuff")
    assert all(("/lds" in k) == (M >= HIER_MIDS["lds"]) and k.endswith("/sync") for k in pin.branches), pin.branches
    return _hier_check(label, dtype, idx, exp, mids_w, deltas, top)


def run_feddyn(label, dtype, layout, order, operands, rounds):
    """Two FedDyn.do rounds (one flame_feddyn_round launch each): average, cld_model and every
    end's history after each round."""
    from flame_amd.optimizers import optimizer_provider
    base, round1, round2 = operands
    idx = {k: index_for(dtype, base[k].numel(), layout) for k in DYN_KEYS}
    opt = optimizer_provider.get("feddyn", alpha=0.1)
    counts = {}
    for r, arr in enumerate((round1, round2)):
        opt.save_state(S._PRE, active_ends=list(DYN_ORDERS[order]))
        assert list(opt.local_param_dict) == DYN_ORDERS[order]
        cache = S.SortedCache()
        for e in arr:
            cache[e] = S.TR({k: place(arr[e][k][idx[k]], layout) for k in DYN_KEYS}, 1)
        src = base if r == 0 else {k: rounds[0][k]["cld"] for k in DYN_KEYS}
        dev_base = {k: place(src[k][idx[k]], layout) for k in DYN_KEYS}
        with Pinned() as pin:
            out = opt.do(dev_base, cache, total=len(arr), num_trainers=len(arr))
        pin.only("flame_feddyn_round")
        for k in DYN_KEYS:
            want = rounds[r][k]
            got = {"avg": out[k], "cld": opt.cld_model[k]}
            exp = {"avg": want["avg"][idx[k]], "cld": want["cld"][idx[k]]}
            for e, h in want["hist"].items():
                assert (h is None) == (opt.local_param_dict[e] is None), (r, e)
                if h is not None:
                    got[f"hist_{e}"], exp[f"hist_{e}"] = opt.local_param_dict[e][k], h[idx[k]]
            check(f"{label}/r{r}/{k}", got, exp)
        zero = rounds[r]["zero"]
        # what was just compared: round 1 averages -0 (round 2 starts from cld, +0); the mean is
        # 0.0 + sum, so cld is +0 in both
        assert bool(torch.signbit(zero["avg"]).all()) == (r == 0) and not bool(torch.signbit(zero["cld"]).any())
        assert not bool(zero["avg"].any()) and not bool(zero["cld"].any())
        for what in ("avg", "cld"):
            counts.setdefault(what, []).append(compared_rows(dtype, rounds[r]["pair"][what]))
        counts.setdefault("hist", []).extend(compared_rows(dtype, h) for h in rounds[r]["pair"]["hist"].values()
                                             if h is not None)
    return counts
