"""flame_agg_reduce_lowrank over one fp32 key just past 2^32 elements (65,537 x 65,537: an element offset i * n + j in 32
bits would wrap): one client of rank 1, integer data, checked exactly on the device in row slices against torch.outer."""
import pytest
import torch

from large_case import DEV, _free, _need

pytestmark = [pytest.mark.gpu]
M, ROWS = 65537, 2048


def _base(lo, hi):       # rows [lo, hi) of the base: integers of [-8, 8] from the 64-bit element offset
    return (torch.arange(lo * M, hi * M, device=DEV, dtype=torch.int64) % 17).float().sub_(8).view(hi - lo, M)


def test_a_key_past_2_32_elements():
    from flame_amd import engine, lowrank
    _need(4 * M * M / 1e9 + 4)
    g = torch.Generator().manual_seed(34)
    u, v = (torch.randint(-8, 9, s, generator=g).float().to(DEV) for s in ((M, 1), (1, M)))
    agg = {"w": torch.empty(M, M, device=DEV)}
    for lo in range(0, M, ROWS):
        agg["w"][lo:lo + ROWS] = _base(lo, min(M, lo + ROWS))
    engine.accumulate(agg, [(lowrank.LowRankWeights({"w": u}, {"w": v}, {"w": (M, M)}), 0.5)])
    for lo, hi in ((lo, min(M, lo + ROWS)) for lo in range(0, M, ROWS)):
        assert torch.equal(agg["w"][lo:hi], _base(lo, hi) + torch.outer(u[lo:hi, 0] * 0.5, v[0])), (lo, hi)
    agg.clear(), _free()
