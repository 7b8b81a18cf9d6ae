"""The restatement of flame_agg_select's contract (tests/select_ref.py) against the two routes of
tests/trimmed_ref.py, without a GPU: on exact-sum inputs the order of the fp64 adds cannot matter,
so ``select`` must equal the sorted definition bit for bit at every (n, k), and the streaming
selection wherever the chain kernel exists (k <= 16)."""
import numpy as np
import pytest
import torch

import select_ref as SR
import trimmed_ref as R

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["f32", "bf16", "f16", "f64"]
NK = [(35, 17), (36, 17), (64, 31), (64, 20), (100, 45), (1025, 512), (1025, 100), (9, 0), (40, 3)]


@pytest.mark.parametrize("nk", NK, ids=[f"n{n}k{k}" for n, k in NK])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_exact_sum_inputs_equal_the_sorted_definition_and_the_stream(dt, nk):
    n, k = nk
    numel = 37 if n > 1000 else 301
    g = torch.Generator().manual_seed(100 * n + k + DTYPES.index(dt))
    xs = R.exact_inputs(g, dt, n, numel)
    base = torch.randn(numel, generator=g).to(dt)
    for b in (base, None):
        got = SR.select(xs, k, b, dt)
        R.same_bits(f"by_sort n={n} k={k}", got, R.by_sort(xs, k, b, dt))
        if k <= 16:
            R.same_bits(f"stream n={n} k={k}", got, R.stream(xs, k, b, dt))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_special_values(dt):
    """20 x [nan, 1, -0, +inf, 2] + 21 x [1, 1, +0, -inf, 2]."""
    a = torch.tensor([float("nan"), 1.0, -0.0, float("inf"), 2.0], dtype=dt)
    b = torch.tensor([1.0, 1.0, 0.0, float("-inf"), 2.0], dtype=dt)
    xs = [a] * 20 + [b] * 21
    for k in (0, 5, 19, 20):
        got = SR.select(xs, k, None, dt)
        R.same_bits(f"k={k}", got, R.by_sort(xs, k, None, dt))
    inf, nan = float("inf"), float("nan")
    R.same_bits("k=19", SR.select(xs, 19, None, dt), torch.tensor([nan, 1.0, 0.0, nan, 2.0], dtype=dt))
    R.same_bits("k=20", SR.select(xs, 20, None, dt), torch.tensor([1.0, 1.0, 0.0, -inf, 2.0], dtype=dt))
    assert R.bits(SR.select(xs, 20, None, dt))[2] == 0                   # +0, not -0


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_radix_search_finds_the_order_statistics(dt):
    """The kernel's search (4-bit digits, MSB first), restated in numpy, equals np.sort on wide
    data, on ties and on keys that differ in one digit only."""
    ut, _, bits, _ = R._U[dt]
    g = torch.Generator().manual_seed(3 + DTYPES.index(dt))
    n = 45
    wide = torch.randn(n, 200, generator=g, dtype=torch.float64) * torch.exp2(torch.rand(n, 200, generator=g, dtype=torch.float64) * 60 - 30)
    xs = [wide[i].to(dt) for i in range(n)]
    for i in range(n):                                                   # columns of ties, specials and near keys
        xs[i][0] = 1.0
        xs[i][1] = float("nan") if i % 3 == 0 else (-0.0 if i % 3 == 1 else 0.0)
        xs[i][2] = float("inf") if i < 22 else float("-inf")
    keys = np.stack([R.to_key(R.bits(x), dt) for x in xs])
    keys[:, 3] = ut(1 << (bits - 1)) + np.arange(n).astype(ut)          # the lowest digits only
    keys[:, 4] = np.where(np.arange(n) % 2 == 0, ut(5), ut((1 << bits) - 6))   # the top digit only
    srt = np.sort(keys, axis=0)
    for rank in (0, 1, 17, 22, 27, 43, 44):
        assert np.array_equal(SR.radix_order_statistic(keys, rank, bits), srt[rank]), rank
