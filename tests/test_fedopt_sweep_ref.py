"""Host: what the FedOPT operand sweeps (tests/test_gpu_fedopt_sweep16.py) expect is what it claims
to be.  The GPU tests compare the kernels with OracleFedOPT, whose 16-bit steps are torch-CPU's own
bf16 / fp16 kernels; here that sequence is checked against a plain reference of the collapsed step
(fedopt_sweep.plain_reference): every op in float64, then ONE round-to-nearest-even to the 16-bit
dtype (round-to-odd into fp32, then the integer rounding on the bits -- never a float64 -> fp32 ->
16-bit double rounding), on every operand the root and quotient sweeps use.  float64 holds the
exact sum and the root / quotient of 16-bit operands to 53 bits, more than twice the 8 / 11 bits of
the target plus two, so the single rounding is the correctly rounded result of each op.

The packings and the sweep lists are checked here too: they decide what the GPU tests cover."""
import pytest
import torch

import fedopt_sweep as F

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
UPPER = {torch.bfloat16: 2.0 ** 38, torch.float16: 2.0 ** 15}
ROOT_TAUS = {dt: [2.0 ** -20, 1e-3, 1.0, UPPER[dt], 2.0 ** -21, 2 * UPPER[dt]] for dt in DTYPES}
MIN_COMPARED = {torch.float16: 31744, torch.bfloat16: 32640}     # the non-negative finite patterns


def _check(label, ref, cur):
    nan = torch.isnan(cur)
    assert torch.equal(torch.isnan(ref), nan), f"{label}: NaN positions differ"
    bad = ((ref.view(torch.int16) != cur.view(torch.int16)) & ~nan).nonzero().flatten()
    assert bad.numel() == 0, (f"{label}: {bad.numel()} elements differ, first at {bad[:4].tolist()}: "
                              f"{ref[bad[:4]].tolist()} (float64, one rounding) vs {cur[bad[:4]].tolist()} (torch-CPU)")
    return int((~nan).sum())


@pytest.mark.parametrize("sort", F.SORTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_root_sweep_expectation_is_the_correctly_rounded_step(dtype, sort):
    src = F.root_source(dtype)
    for tau in ROOT_TAUS[dtype]:
        cur, _, _ = F.oracle_collapsed(sort, tau, src)
        n = _check(f"{sort}/tau={tau}", F.plain_reference(src.m, src.v, tau, dtype)[:src.n], cur[:src.n])
        assert n >= MIN_COMPARED[dtype], (tau, n)


@pytest.mark.parametrize("tau", [2.0 ** -20, 1e-3, 1.0, "upper"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_quotient_sweep_expectation_is_the_correctly_rounded_step(dtype, tau):
    """Every numerator x every v of the quotient sweep.  One variant: under the collapse the three
    run the same root and quotient ops (test_root_sweep... runs all three)."""
    tau = UPPER[dtype] if tau == "upper" else tau
    src = F.quotient_source(dtype)
    cur, _, _ = F.oracle_collapsed("fedyogi", tau, src)
    n = _check(f"tau={tau}", F.plain_reference(src.m, src.v, tau, dtype)[:src.n], cur[:src.n])
    required = ~torch.isnan(src.m[:src.n]) & ~torch.signbit(src.v[:src.n])
    assert n >= int(required.sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_single_rounding_differs_from_double_rounding(dtype):
    """round_f64_to rounds once: a value just above a 16-bit midpoint by less than half an fp32 ulp
    goes up, where float64 -> fp32 -> 16-bit lands on the midpoint and ties down to even."""
    ulp = 2.0 ** -F.MANT_BITS[dtype]
    x = 1.0 + ulp / 2 + 2.0 ** -40
    once = float(F.round_f64_to([x, -x, 1.0 + ulp / 2, 1.0 + 3 * ulp / 2], dtype)[0])
    assert once == 1.0 + ulp
    assert float(torch.tensor(x, dtype=torch.float64).float().to(dtype)) == 1.0            # the double rounding
    got = F.round_f64_to([x, -x, 1.0 + ulp / 2, 1.0 + 3 * ulp / 2, float("inf"), 1e300, -1e-300, 0.0], dtype)
    assert got.tolist() == [1.0 + ulp, -1.0 - ulp, 1.0, 1.0 + 2 * ulp, float("inf"), float("inf"), -0.0, 0.0]
    assert bool(torch.signbit(got[6]))
    every = F.all_patterns16(dtype)
    back = F.round_f64_to(every.double().numpy(), dtype)
    keep = ~torch.isnan(every)
    assert torch.equal(back.view(torch.int16)[keep], every.view(torch.int16)[keep])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_quotient_v_list(dtype):
    """+0, the smallest and the largest subnormal, every binade of normals up to the largest admitted
    v, and all three mantissa kinds."""
    mb, top = F.MANT_BITS[dtype], F.V_TOP[dtype]
    vb = F.quotient_v_bits(dtype)
    assert len(vb) == len(set(vb)) == F.V_COUNT[dtype]
    assert {0, 1, (1 << mb) - 1} <= set(vb) and max(vb) == top and min(vb) == 0
    assert {b >> mb for b in vb} == set(range(0, (top >> mb) + 1))
    normal = [b for b in vb if b >> mb]
    ones = (1 << mb) - 1
    assert sum(b & ones == 0 for b in normal) >= 30 and sum(b & ones == ones for b in normal) >= 30
    assert sum(b & ones not in (0, ones) for b in normal) >= 30
    assert vb == F.quotient_v_bits(dtype)          # seeded


@pytest.mark.parametrize("lane", [8, 4])
@pytest.mark.parametrize("packing", F.PACKINGS)
def test_packings(packing, lane):
    n, chunk = 1000, 256
    src, is_sweep = F.pack_index(n, packing, lane, chunk)
    assert src.numel() % chunk == 0
    assert torch.equal(src[is_sweep], torch.arange(n))             # every sweep entry once, in order
    lanes = src.view(-1, lane)
    poisoned = (lanes == n).sum(1)
    full = (lanes < n).all(1) | ((lanes < n).sum(1) == lane - 1) & (poisoned == 1)
    k = int(full.sum())                                             # the lanes before the padded tail
    assert k >= n // lane and bool(full[:k].all())
    if packing == "pure":
        assert int(poisoned.sum()) == 0
    elif packing == "poisoned":
        assert bool((poisoned[:k] == 1).all())
        assert len({int((row == n).nonzero()[0]) for row in lanes[:k]}) == lane    # every slot takes a turn
    else:
        assert bool((poisoned[:k:2] == 0).all()) and bool((poisoned[1:k:2] == 1).all())
        wave = poisoned[:64 * (k // 64)].view(-1, 64)               # both kinds in every wave of 64 lanes
        assert bool(((wave == 0).any(1) & (wave == 1).any(1)).all())
    assert int(poisoned[k + 1:].sum()) == 0
    assert F.sweep_capacity(packing, lane, k * lane) <= n + lane


def test_moment_states_hold_the_named_values():
    for dtype in DTYPES:
        m, v = F.moment_states(dtype)
        assert m.numel() == v.numel() == 64
        fi = torch.finfo(dtype)
        sub = F.from_bits([1], dtype)[0]
        for t in (m, v):
            bits = set(t.view(torch.int16).tolist())
            for want in (0.0, -0.0, float(sub), fi.max, float("inf"), float("-inf")):
                assert int(torch.tensor(want, dtype=dtype).view(torch.int16)) in bits, (dtype, want)
            assert bool(torch.isnan(t).any())
        d = torch.tensor([2.0, 0.5, 2.0 ** -7, 3.0, 1.0], dtype=dtype)
        assert all(bool((v == x * x).any()) for x in d)              # v - d^2 exactly 0 for some d
