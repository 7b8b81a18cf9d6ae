"""Host: what the aggregation sweeps (tests/test_gpu_agg_sweep16.py, tests/test_gpu_agg_sweep_wide.py)
expect is what it claims to be, and it leaves enough to compare.

The GPU tests hold the kernels to the torch-CPU restatement of the reference's statements
(tests/agg_sweep.py).  Here the four ops of that restatement -- the product, the sum, the quotient
and the difference -- are held to a plain numpy reference on every operand list of the sweeps: the
exact op in float64, rounded to fp32, then to the 16-bit dtype (``astype(np.float16)``; an integer
round-to-nearest-even on the fp32 bits for bf16).  float64 is a valid reference: on fp32-representable
inputs each of the four ops is double-rounding safe from 53 to 24 bits (Figueroa: 53 >= 2 * 24 + 2),
so the float64 result rounded to fp32 IS the fp32 op, which is what torch-CPU rounds to 16 bits.

The floors: a NaN expectation is compared as "NaN meets NaN" only, so every case the GPU tests run
must keep at least agg_sweep.FLOOR = 60,000 non-NaN expectations in each row of 65,536 patterns (the
same share of an f32 / f64 grid row).  A delta over an infinite base is NaN everywhere (inf - inf)
and exempt.  The measured minima are printed; DESIGN.md records them."""
import numpy as np
import pytest
import torch

import agg_sweep as A
import fedopt_sweep as F

DT16 = list(A.DTYPES16.items())
DT_ALL = DT16 + list(A.DTYPES_WIDE.items())
ids = lambda cases: [n for n, _ in cases]


def to_dtype(x, dtype):
    """float64 -> fp32 -> the dtype, each step round-to-nearest-even."""
    with np.errstate(all="ignore"):
        if dtype == torch.float64:
            return torch.from_numpy(np.asarray(x, dtype=np.float64))
        f = np.asarray(x, dtype=np.float64).astype(np.float32)
        if dtype == torch.float32:
            return torch.from_numpy(f)
        if dtype == torch.float16:
            return torch.from_numpy(f.astype(np.float16))
        b = f.view(np.uint32).astype(np.uint64)
        r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
        r[np.isnan(f)] = 0x7FC0
        return torch.from_numpy(r.view(np.int16)).view(torch.bfloat16)


def f64(t):
    return t.to(torch.float64).numpy()


def scalar(x, dtype):
    """A Python scalar as torch hands it to the op: fp32 for f32 and the 16-bit dtypes, a double for f64."""
    return float(x) if dtype == torch.float64 else float(np.float32(x))


def same(label, ref, got):
    nan = torch.isnan(got)
    assert torch.equal(torch.isnan(ref), nan), f"{label}: NaN positions differ"
    it = F.INT[got.dtype]
    bad = ((ref.view(it) != got.view(it)) & ~nan).nonzero().flatten()
    assert bad.numel() == 0, (f"{label}: {bad.numel()} elements differ, first at {bad[:4].tolist()}: "
                              f"{ref[bad[:4]].tolist()} (float64 reference) vs {got[bad[:4]].tolist()} (torch-CPU)")


@pytest.mark.parametrize("name,dtype", DT_ALL, ids=ids(DT_ALL))
def test_product(name, dtype):
    """RN(v * rate) on every pattern under every rate and scale, and the scaled reduction's chain."""
    v = A.patterns(dtype)
    with np.errstate(all="ignore"):
        for r in A.RATES + A.SCALES + A.INT_RATES:
            same(f"{name} v * {r}", to_dtype(f64(v) * scalar(r, dtype), dtype), (v * r).to(dtype))
        for s in A.SCALES:
            for r in A.rate_triple(A.SCALES.index(s)):
                ref = to_dtype(f64(to_dtype(f64(v) * scalar(s, dtype), dtype)) * scalar(r, dtype), dtype)
                same(f"{name} (v * {s}) * {r}", ref, (torch.mul(v, s) * r).to(dtype))


@pytest.mark.parametrize("name,dtype", DT_ALL, ids=ids(DT_ALL))
def test_sum_and_difference(name, dtype):
    """RN(acc + v) and RN(v - acc) on every accumulator x every pattern (every block)."""
    for block in range(A.accumulators(dtype).shape[0]):
        acc, pat = A.pair(dtype, block)
        with np.errstate(all="ignore"):
            same(f"{name} acc + v, block {block}", to_dtype(f64(acc) + f64(pat), dtype), acc + pat)
            same(f"{name} v - acc, block {block}", to_dtype(f64(pat) - f64(acc), dtype), pat - acc)


@pytest.mark.parametrize("name,dtype", DT_ALL, ids=ids(DT_ALL))
def test_quotient(name, dtype):
    """RN(a / goal) on every pattern under every goal; then w + q and w' - w as the scale_add
    restatement forms them.  2^24 + 1 is no fp32 value: torch hands the op fp32(goal) = 2^24."""
    a = A.patterns(dtype)
    for goal in A.GOALS:
        with np.errstate(all="ignore"):
            same(f"{name} a / {goal}", to_dtype(f64(a) / scalar(goal, dtype), dtype), a / goal)
            w, ap, new, delta = A.scale_add_case(dtype, goal)
            q = f64(to_dtype(f64(ap) / scalar(goal, dtype), dtype))
            ref_new = to_dtype(f64(w) + q, dtype)
            same(f"{name} w + a / {goal}", ref_new, new)
            same(f"{name} delta, goal {goal}", to_dtype(f64(ref_new) - f64(w), dtype), delta)


@pytest.mark.parametrize("name,dtype", DT16, ids=ids(DT16))
def test_rates_that_tell_one_rounding_from_two(name, dtype):
    """torch rounds the fp32 product to 16 bits: two roundings.  A kernel that rounds the exact
    product once (what v_fma_mixlo_f16 does) differs only where the fp32 rounding lands on a 16-bit
    midpoint, and whether any of the 65,536 values does so depends on the rate: none under 1/3,
    1/sqrt(2), 1/sqrt(3) or any power of two, some under 1e-3 and under 1/6.  So the reduction's
    rate list catches it through 1e-3, and the hierarchy and FedDyn cases carry a rate of 1/6
    (agg_sweep.STALE, the idle ends of agg_sweep.DYN_ORDERS) for it."""
    v = A.patterns(dtype)

    def differ(r):
        r = float(r)
        with np.errstate(all="ignore"):
            once = F.round_f64_to(f64(v) * scalar(r, dtype), dtype)
        twice = (v * r).to(dtype)
        return int(((once.view(torch.int16) != twice.view(torch.int16)) & ~torch.isnan(twice)).sum())

    assert [differ(r) for r in (1.0, 0.5, 1 / 3, 1 / np.sqrt(2), 1 / np.sqrt(3))] == [0] * 5
    some = {r: differ(float(r)) for r in (1e-3, 1 / 6, 1 / np.sqrt(1 + A.STALE), 1 / len(A.DYN_ORDERS["arrival"]))}
    print(f"{name}: values whose product rounds differently once and twice: {some}")
    assert all(n > 0 for n in some.values()), some
    assert 1e-3 in A.RATES and 1 / np.sqrt(1 + A.STALE) == 1 / 6


# ------------------------------------------------------------------ the floors
def _min_rows(dtype, exp, keep=None):
    rows = A.compared_rows(dtype, exp)
    return int((rows if keep is None else rows[keep]).min())


def _floors(dtype):
    """{case: the fewest non-NaN expectations of a row of patterns} over every case the GPU tests run."""
    out = {}
    for i, init, n in A.product_launches(dtype):
        _, _, exp = A.product_case(dtype, i, init, n)
        out[f"product/{i}/{'init' if init else 'acc'}/{n}"] = min(_min_rows(dtype, e) for e in exp)
    for i in range(len(A.RATES) if not A.wide(dtype) else 4):
        *_, exp = A.scaled_case(dtype, i)
        out[f"scaled/{i}"] = min(_min_rows(dtype, e) for e in exp)
    for block in range(A.accumulators(dtype).shape[0]):
        out[f"sum/{block}"] = _min_rows(dtype, A.sum_case(dtype, block)[2])
    out["scaled/pair"] = _min_rows(dtype, A.scaled_pair_case(dtype)[2])
    for goal in A.GOALS:
        w, _, new, delta = A.scale_add_case(dtype, goal)
        fin = A.finite_rows(dtype, A.scale_add_block(dtype, goal))
        out[f"scale_add/{goal}/w"] = _min_rows(dtype, new)
        out[f"scale_add/{goal}/delta"] = _min_rows(dtype, delta, fin)
        assert bool(torch.isnan(delta.view(fin.numel(), -1)[~fin]).all())        # the exempt rows: inf - inf
    if dtype != torch.float64:
        for kind, M in A.HIER_MIDS.items():
            for sync in (False, True):
                for from_none in ((True,) if sync else (True, False)):
                    o, exp = A.hier_expected(dtype, M, sync, from_none)
                    tag = f"hier/{kind}/{'sync' if sync else 'fedbuff'}/{'none' if from_none else 'accum'}"
                    for s in range(A.HIER_SEGS):
                        poisoned = s == A.INF_MID[0]
                        for m in range(M):
                            if poisoned and m == A.INF_MID[1]:
                                assert bool(torch.isnan(exp["delta"][s][m]).all())
                                continue
                            out[f"{tag}/mid_w"] = min(out.get(f"{tag}/mid_w", 1 << 30), _min_rows(dtype, exp["mid_w"][s][m]))
                            out[f"{tag}/delta"] = min(out.get(f"{tag}/delta", 1 << 30), _min_rows(dtype, exp["delta"][s][m]))
                        for nm in ("top_agg", "top_w"):
                            if nm not in exp:
                                continue
                            if poisoned:         # a NaN delta reaches the top: everywhere, and nowhere else
                                assert bool(torch.isnan(exp[nm][s]).all())
                            else:
                                out[f"{tag}/{nm}"] = min(out.get(f"{tag}/{nm}", 1 << 30), _min_rows(dtype, exp[nm][s]))
    for order in A.DYN_ORDERS:
        _, rounds = A.feddyn_expected(dtype, order)
        for r, rd in enumerate(rounds):
            for what in ("avg", "cld"):
                out[f"feddyn/{order}/r{r}/{what}"] = _min_rows(dtype, rd["pair"][what])
            for e, h in rd["pair"]["hist"].items():
                if h is not None:           # (p, q and r never arrive)
                    out[f"feddyn/{order}/r{r}/hist_{e}"] = _min_rows(dtype, h)
    return out


@pytest.mark.parametrize("name,dtype", DT_ALL, ids=ids(DT_ALL))
def test_every_case_keeps_the_floor(name, dtype):
    floors = _floors(dtype)
    n = A.patterns(dtype).numel()
    worst = min(floors, key=floors.get)
    for case, least in sorted(floors.items()):
        print(f"{name} {case}: compared at least {least} of {n} per row")
    print(f"{name}: minimum over all cases {floors[worst]} of {n} ({worst}), floor {A.floor(dtype)}")
    short = {c: v for c, v in floors.items() if v < A.floor(dtype)}
    assert not short, short


# ------------------------------------------------------------------ the lists
@pytest.mark.parametrize("name,dtype", DT_ALL, ids=ids(DT_ALL))
def test_accumulator_list(name, dtype):
    acc = A.accumulators(dtype)
    mb = F.MANT_BITS[dtype]
    assert acc.shape[1] == A.rows(dtype) and not bool(torch.isnan(acc).any())
    fi = torch.finfo(dtype)
    sub = float(F.from_bits([1], dtype)[0])
    sub_max = float(F.from_bits([(1 << mb) - 1], dtype)[0])
    for block in acc:
        vals = block.tolist()
        for want in (sub, sub_max, fi.max, -fi.max, float("inf"), float("-inf")):
            assert want in vals, (name, want)
        zeros = block[block == 0]
        assert zeros.numel() == 2 and bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())
        assert int(torch.signbit(block).sum()) >= A.rows(dtype) // 4          # both signs
    bits = acc.view(F.INT[dtype]).flatten().numpy().astype(np.int64) & (A.sign_bit(dtype) - 1)
    binades = set((bits >> mb).tolist())
    if not A.wide(dtype):
        assert binades == set(range(0, (A.inf_bits(dtype) >> mb) + 1)), name       # every binade, 0 and inf's too
        mant = bits[(bits >> mb > 0) & (bits < A.inf_bits(dtype))] & ((1 << mb) - 1)
        ones = (1 << mb) - 1
        assert (mant == 0).sum() >= 8 and (mant == ones).sum() >= 8 and ((mant != 0) & (mant != ones)).sum() >= 8
    else:
        assert len(binades) >= 10
    assert torch.equal(acc.view(F.INT[dtype]), A.accumulators.__wrapped__(dtype).view(F.INT[dtype]))     # seeded


@pytest.mark.parametrize("name,dtype", DT_ALL, ids=ids(DT_ALL))
def test_permutations_stay_in_the_binade(name, dtype):
    p = A.patterns(dtype)
    n = p.numel()
    assert n == (1 << 16 if not A.wide(dtype) else 2 * 16 << A.EXP_BITS[dtype])
    mb = F.MANT_BITS[dtype]
    bits = A.pattern_bits(dtype)
    assert np.unique(bits).size == n
    field = lambda b: (b >> np.uint64(mb)) & np.uint64((1 << A.EXP_BITS[dtype]) - 1)
    for k in (1, 2, 7, 8, 40):
        perm = A.permutation(dtype, k)
        assert torch.equal(torch.sort(perm).values, torch.arange(n))
        q = p[perm]
        assert torch.equal(torch.isnan(q), torch.isnan(p)) and torch.equal(torch.isinf(q), torch.isinf(p))
        assert (field(bits[perm.numpy()]) == field(bits)).all()
        keep = ~torch.isnan(p)
        assert torch.equal(torch.signbit(q)[keep], torch.signbit(p)[keep] ^ bool(k % 2))
        assert int((q.view(F.INT[dtype]) != p.view(F.INT[dtype])).sum()) > n // 2


def test_layouts():
    for n, lane, chunk in ((1 << 16, 8, 2048), (8192, 4, 1024), (1000, 2, 512)):
        mis = A.layout_index(n, "misaligned", lane, chunk)
        assert torch.equal(mis, torch.arange(n))
        al = A.layout_index(n, "aligned", lane, chunk)
        assert al.numel() % chunk == lane - 1 and al.numel() > chunk and torch.equal(al[:n], mis)
        assert int(al.max()) < n and torch.unique(al[-(lane - 1):]).numel() == lane - 1


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_integer_pairs(dtype):
    """+-2^k and +-(2^k +- 1); at least 90 % of the value x rate pairs have a product that fits the
    type; the restatement equals the exact arithmetic: trunc(fp32(fp32(v) * fp32(rate))), wrapping add."""
    v, base, rates, keep, exp = A.int_case(dtype)
    top = A.INT_TOP[dtype]
    vals = set(v.tolist())
    assert all(s * (2 ** k + d) in vals for k in (0, 24, 25, top) for d in (-1, 0, 1) for s in (1, -1))
    kept = sum(int(k.sum()) for k in keep)
    assert kept >= 0.9 * len(rates) * v.numel(), (kept, len(rates) * v.numel())
    bits = 8 * v.element_size()
    for r, k, e in zip(rates, keep, exp):
        # fp32(v) x fp32(rate): exact in float64, rounded to fp32
        prod =(v.numpy().astype(np.float32).astype(np.float64) * float(np.float32(r))).astype(np.float32)
        want = []
        for b, p, ok in zip(base.tolist(), prod.tolist(), k.tolist()):
            if ok:
                s = (b + int(p)) & ((1 << bits) - 1)                  # int(): toward zero
                want.append(s - (1 << bits) if s >> (bits - 1) else s)
        assert e[k].tolist() == want, (dtype, r)
        if r < 0 or r not in (1.0,):
            assert any(p != int(p) for p in prod.tolist())            # truncation happens
