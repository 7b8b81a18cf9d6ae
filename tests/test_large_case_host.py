"""CPU: what keeps tests/test_gpu_large_kernels.py from passing vacuously (no GPU, no mutation build:
a narrowed index on the device is an out-of-bounds access by construction).

* The sample set holds every boundary and the whole tail past 2^32; for P32 it is the set
  tests/test_gpu_large.py has always used.
* A kernel whose element index wrapped at 2^32 (unsigned) or 2^31 would read an input at
  ``e - 2^32`` / ``e - 2^31``.  For the sampled rows whose result could plausibly survive that --
  the fp32 sum of bf16 clients, the median of 3 -- the reference recomputed from such inputs must
  differ from the true one at no fewer than 99 % of the samples behind the boundary, whether the
  clients, the base or both are read early.  Measured: 0.9968-0.9989 for the median of 3 over a base
  of sigma 1e-2, 0.9998-1.0 for the fp32 sum.  (A base of sigma 1.0 would swallow the change in its
  bf16 ulp: only 82 % of the medians differ.)
* The exact-integer recipe of the reductions stays exact, and the sentinels name their positions.
"""
import numpy as np
import pytest
import torch

import large_case as LC
import select_ref as SR
import trimmed_ref as R
import uplink16_case as U

BF16, F32 = torch.bfloat16, torch.float32


def test_index_p32_is_the_set_the_parent_file_used():
    P = LC.P32
    edges = []
    for b in (0, 1 << 30, (1 << 31) - 2048, 1 << 31, P - 4099, P - 2048):
        edges += list(range(max(0, b - 3), min(P, b + 3)))
    edges += [1023, 1024, 1025, 2047, 2048, P - 1]
    rand = np.random.default_rng(0).integers(0, P, 20_000)
    want = torch.from_numpy(np.unique(np.concatenate([np.array(edges), rand])).astype(np.int64))
    assert torch.equal(LC.index(P), want)


def test_index_p16_holds_every_boundary_and_the_whole_tail():
    P = LC.P16
    assert P == 2 ** 32 + 70_001 and P - 2 ** 32 == 34 * 2048 + 369
    idx = LC.index(P).numpy()
    assert idx.dtype == np.int64 and np.all(np.diff(idx) > 0) and idx[0] == 0 and idx[-1] == P - 1
    have = set(idx.tolist())
    for b in (0, 1 << 30, 1 << 31, 1 << 32, (1 << 31) - 2048, (1 << 31) + 2048, (1 << 32) - 4096, (1 << 32) - 2048,
              (1 << 32) - 1024, (1 << 32) + 2048, (1 << 32) + 4096, (1 << 32) + 34 * 2048):
        for e in range(max(0, b - 3), b + 3):
            assert e in have, (b, e)
    tail = idx[idx >= 1 << 32]
    assert tail.size == 70_001 and tail[0] == 1 << 32 and tail[-1] == P - 1
    # 20,000 uniform samples alone leave the tail nearly empty: it has to be taken whole
    assert int((np.random.default_rng(0).integers(0, P, 20_000) >= 1 << 32).sum()) < 20
    assert int(((idx >= 1 << 31) & (idx < 1 << 32)).sum()) > 9_000


def _behind(idx, shift):
    """The samples a wrap by ``shift`` would corrupt, and where it would read instead."""
    if shift == 1 << 32:
        e = idx[idx >= 1 << 32]
    else:
        e = idx[(idx >= 1 << 31) & (idx < 1 << 32)]
    return e, e - shift


def _differs(a, b):
    return float((torch.from_numpy(R.bits(a) != R.bits(b))).double().mean())


@pytest.mark.parametrize("wrapped", ["clients", "base", "all"])
@pytest.mark.parametrize("shift", [1 << 32, 1 << 31], ids=["2^32", "2^31"])
@pytest.mark.parametrize("row", ["mixed", "trimmed", "select"])
def test_a_wrapped_index_would_show(row, shift, wrapped):
    """Rows 2, 4 and 5 on their own inputs: the reference from inputs read ``shift`` elements early
    differs from the true reference at >= 99 % of the samples behind the boundary."""
    e, w = _behind(LC.index(LC.P16), shift)
    assert e.numel() > 9_000
    if row == "mixed":
        n, bdt, sigma = 2, F32, 1.0

        def ref(b, us):
            return U.restate(b, us, LC.RATES)
    else:
        n, bdt, sigma = 3, BF16, LC.ROBUST_BASE_SIGMA

        def ref(b, us):
            return (R.stream if row == "trimmed" else SR.select)(us, 1, b, BF16)
    b_true, u_true = LC.case_host(LC.SEED[row], e, n, sigma, bdt, BF16)
    b_wrap, u_wrap = LC.case_host(LC.SEED[row], w, n, sigma, bdt, BF16)
    true = ref(b_true, u_true)
    got = ref(b_wrap if wrapped in ("base", "all") else b_true, u_wrap if wrapped in ("clients", "all") else u_true)
    frac = _differs(got, true)
    print(f"{row} shift {shift} wrapped {wrapped}: {frac:.4f} of {e.numel()} samples differ")
    assert frac >= 0.99, (row, shift, wrapped, frac)


def test_exact_integer_recipe():
    """The dense recipe gives integers of [-8, 8] that bf16 holds exactly, mostly non-zero; the sums
    stay far below 2^53; the sentinels' squares are six distinct powers of 4."""
    assert LC.DENSE_MAX ** 2 * LC.P16 < 2 ** 39 < 2 ** 53
    assert (2 * LC.DENSE_MAX) ** 2 * LC.P16 < 2 ** 53                # |x - z| <= 16: the distances too
    idx = LC.index(LC.P16)
    x = LC.integer_valued(LC.host_synth(LC.SEED["stats"], 1, idx,LC.DENSE_SIGMA, BF16))
    xd = x.double()
    assert x.dtype == BF16 and torch.equal(xd, xd.round()) and float(xd.abs().max()) <= LC.DENSE_MAX
    assert torch.equal(x.float().bfloat16().double(), xd)
    assert 8.0 < float((xd * xd).mean()) < 10.0 and float((xd != 0).double().mean()) > 0.8
    sq = [v * v for v in LC.SENTINEL_VALUES]
    assert sq == [4 ** j for j in range(6)] and len(set(sq)) == 6 and sum(sq) == 0b010101010101
    pos = LC.sentinels(LC.P16)
    assert pos == sorted(set(pos)) and pos[-1] == LC.P16 - 1
    assert {p for p in pos} >= {(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32}


def test_host_synth_formats():
    """host_synth's 16-bit roundings are torch's (round to nearest even from the fp32 value)."""
    idx = torch.arange(0, 70_001, dtype=torch.int64) + ((1 << 32) - 35_000)
    x = LC.host_synth(5, 3, idx, 1.0)
    assert torch.equal(LC.host_synth(5, 3, idx, 1.0, BF16).view(torch.int16), x.bfloat16().view(torch.int16))
    assert torch.equal(LC.host_synth(5, 3, idx, 1.0, torch.float16).view(torch.int16), x.half().view(torch.int16))
    assert torch.equal(LC.host_synth(5, 3, idx, 1.0, torch.float64), x.double())
