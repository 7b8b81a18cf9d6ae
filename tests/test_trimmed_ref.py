"""The test-side restatement of the trimmed mean (tests/trimmed_ref.py) against itself, without a
GPU: the streaming procedure equals the sort-based definition bit for bit on exact-sum inputs, and
the integer key map is monotone and round-trips.

Exact-sum inputs: x = m * 2^-24 with integer |m| < 2^24 (f32 / f64), integers in [-8, 8] (bf16 /
f16).  Every partial sum of up to 4,096 such values is a multiple of 2^-24 below 2^12, exact in
fp64, so the order the kept values are added in cannot matter and ``stream`` must equal
``by_sort``.  Planted NaN / +-inf / -0 keep that: any order gives the same NaN / inf / sign.
"""
import numpy as np
import pytest
import torch

import trimmed_ref as R

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["f32", "bf16", "f16", "f64"]
SHAPES = [(1, 0), (3, 1), (5, 2), (9, 1), (9, 4), (33, 16), (70, 8), (7, 0), (8, 3), (34, 16)]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stream_equals_by_sort_on_exact_sums(dt):
    g = torch.Generator().manual_seed(7 + DTYPES.index(dt))
    for n, k in SHAPES:
        xs = R.exact_inputs(g, dt, n, 301)
        for planted in (False, True):
            if planted:
                for i, v in enumerate([float("nan"), float("inf"), float("-inf"), -0.0, -float("nan")]):
                    for c in range(min(n, i + 2)):          # the value at i + 2 clients of one stretch
                        xs[(c * 5 + i) % n][i * 40:i * 40 + 7] = v
            base = torch.randn(301, generator=g).to(dt)
            for b in (base, None):
                s, d = R.stream(xs, k, b, dt), R.by_sort(xs, k, b, dt)
                assert s.dtype == dt and s.shape == (301,)
                R.same_bits(f"{dt} n={n} k={k} planted={planted} base={b is not None}", s, d)
            if dt == torch.float32:
                # the definition once more through torch.sort (NaN last), summed in fp64 and divided
                kept = torch.sort(torch.stack(xs), 0).values[k:n - k].double()
                acc = torch.zeros(301, dtype=torch.float64)
                for row in kept:
                    acc = acc + row
                R.same_bits(f"torch.sort n={n} k={k}", R.stream(xs, k, base, dt), base + (acc / (n - 2 * k)).float())


def _check_map(u, dt):
    key = R.to_key(u, dt)
    assert np.array_equal(R.from_key(key, dt), u), "round trip"
    x = R.from_bits(u, dt).double().numpy()
    order = np.argsort(key, kind="stable")
    xs, ks, us = x[order], key[order], u[order]
    assert np.all(xs[1:] >= xs[:-1]), "keys order the values"
    same_val = xs[1:] == xs[:-1]
    # equal values with different keys: only -0 before +0
    differ = same_val & (ks[1:] != ks[:-1])
    assert np.all(xs[1:][differ] == 0.0) and np.all(np.signbit(R.from_bits(us[:-1][differ], dt).double().numpy()))
    assert np.all(ks[1:][~same_val] > ks[:-1][~same_val]), "strictly monotone on distinct values"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_key_map_every_16_bit_pattern(dt):
    u = np.arange(1 << 16, dtype=np.uint16)
    x = R.from_bits(u, dt)
    finite = torch.isfinite(x).numpy()
    _check_map(u[finite], dt)
    nan = torch.isnan(x).numpy()
    assert nan.sum() > 0 and np.all(R.to_key(u[nan], dt) == 0xFFFF)        # every NaN, either sign: the all-ones key
    back = R.from_bits(R.from_key(np.array([0xFFFF], np.uint16), dt), dt)
    assert bool(torch.isnan(back).all()) and int(R.from_key(np.array([0xFFFF], np.uint16), dt)[0]) == 0x7FFF   # a quiet NaN
    inf = R.to_key(R.bits(torch.tensor([float("-inf"), float("inf")]).to(dt)), dt)
    assert inf[0] == R.to_key(u[finite], dt).min() - 1 and inf[1] == R.to_key(u[finite], dt).max() + 1 and inf[1] < 0xFFFF


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_key_map_random_values(dt):
    rng = np.random.default_rng(11)
    ut = np.uint32 if dt == torch.float32 else np.uint64
    u = rng.integers(0, np.iinfo(ut).max, size=1_000_000, dtype=ut, endpoint=True)
    x = R.from_bits(u, dt)
    finite = torch.isfinite(x).numpy()
    edge = R.bits(torch.tensor([0.0, -0.0, torch.finfo(dt).tiny / 4, -torch.finfo(dt).tiny / 4, torch.finfo(dt).max,
                                torch.finfo(dt).min], dtype=torch.float64).to(dt))
    _check_map(np.concatenate([u[finite], edge]), dt)
    ones = ut(np.iinfo(ut).max)
    nans = R.bits(torch.tensor([float("nan"), -float("nan")], dtype=dt))
    assert np.all(R.to_key(nans, dt) == ones) and np.all(R.to_key(u[~finite & torch.isnan(x).numpy()], dt) == ones)
    assert bool(torch.isnan(R.from_bits(R.from_key(np.array([ones], ut), dt), dt)).all())
    lo, hi = R.to_key(R.bits(torch.tensor([float("-inf"), float("inf")], dtype=dt)), dt)
    keys = R.to_key(u[finite], dt)
    assert lo < keys.min() and keys.max() < hi < ones
