"""flame_lowrank_factor on the host: the symbols resolve, the launch-branch table and the ABI version are unchanged, every
refusal carries its code and names the entry point before any HIP call, the planner splits K as the header says, and
lowrank.apply_ is densify added to the model.  No GPU call."""
import ctypes

import numpy as np
import pytest
import torch

from flame_amd import _native as N
from flame_amd import engine, lowrank
from test_abi import header_functions

WHO = b"flame_lowrank_factor"
NAMES = {"flame_lowrank_factor", "flame_lowrank_factor_scratch_bytes"}


def test_symbols_sizes_and_refusals():
    L, FAKE, err = N.lib(), ctypes.c_void_p(4096), N.lib().flame_last_error     # FAKE is never dereferenced
    assert NAMES <= set(N.EXPORTS) and NAMES <= set(header_functions()) and all(hasattr(L, n) for n in NAMES)
    assert L.flame_launch_branches() == 100 and L.flame_abi_version() == 1 and not any("factor" in n for n in N.launch_branch_counts())
    # one 128 x 32 fp32 partial per work item of the larger pass
    assert [L.flame_lowrank_factor_scratch_bytes(*a) for a in ((3, 5), (5, 3), (0, 5), (5, 0), (2 ** 24, 1))] == [5 * 16384, 5 * 16384, 0, 0, 0]
    need = L.flame_lowrank_factor_scratch_bytes(3, 5)
    args = {"flags": 0, "segs": FAKE, "n_segs": 1, "rank": 16, "max_elems": 1 << 20, "p": 3, "v": 5, "scratch": FAKE, "bytes": need}
    call = lambda **kw: L.flame_lowrank_factor(*{**args, **kw}.values(), None)      # noqa: E731
    for kw, text in (({"segs": None}, b"segment"), ({"n_segs": 0}, b"segment"), ({"n_segs": -1}, b"segment"), ({"rank": 0}, b"rank 0"),
                     ({"rank": 33}, b"rank 33"), ({"rank": -1}, b"rank -1"), ({"flags": 1}, b"unknown flags"), ({"flags": 1 << 20}, b"unknown flags"),
                     ({"max_elems": -1}, b"max_elems"), ({"p": 0}, b"work items"), ({"v": 2 ** 24}, b"work items"),
                     ({"scratch": None}, b"scratch"), ({"bytes": need - 1}, b"%d needed" % need)):
        assert call(**kw) == N.FLAME_EINVAL and WHO in err() and text in err(), (kw, err())
    for big in (2 ** 31, 2 ** 40):
        assert call(max_elems=big) == N.FLAME_ENOTSUP and WHO in err() and b"2^31" in err()


def test_plan_splits_k_by_the_shapes_alone():
    seg = lambda m, n, r: (16, 32, 48, 64, 80, m, n, r, r, 1)      # noqa: E731
    meta, p_items, v_items, big = engine.plan_lowrank_factor([seg(257, 130, 4), seg(1, 4096, 1)], tile=128, items=16)
    head = meta.reshape(2, N.LOWRANK_FACTOR_SEGMENT_INT64S)
    # P: 3 + 1 tiles share 16 items: 4 splits each where K has the stages (130 columns are 3 stages: 3 splits of one)
    assert head[:, 10:13].tolist() == [[0, 3, 64], [9, 4, 1024]] and p_items == 13
    # V: 2 + 32 tiles: one split each, K = m whole
    assert head[:, 13:16].tolist() == [[0, 1, 320], [2, 1, 64]] and v_items == 34 and big == 257 * 130
    assert head[0, :10].tolist() == [16, 32, 48, 64, 80, 257, 130, 4, 4, 1]
    for bad in (seg(0, 4, 1), seg(4, 4, 5), seg(64, 64, 33), seg(4, 4, 0), seg(2 ** 16, 2 ** 15, 4)):
        with pytest.raises(ValueError, match="plan_lowrank_factor"):
            engine.plan_lowrank_factor([bad], tile=128)
    with pytest.raises(RuntimeError, match="lowrank_factor"):
        engine.lowrank_factor({"w": torch.zeros(4, 4)}, 2, base={}, device="cpu")


def test_apply_is_densify_added():
    g = torch.Generator().manual_seed(5)
    u, v, b = torch.randn(6, 2, generator=g), torch.randn(2, 20, generator=g), torch.randn(6, 4, 5, generator=g)
    msg = lowrank.LowRankWeights({"w": u, "steps": torch.tensor([7])}, {"w": v}, {"w": (6, 4, 5)})
    model = {"w": b.clone(), "steps": torch.tensor([3])}
    assert lowrank.apply_(model, msg) is model and model["steps"].item() == 7
    assert torch.equal(model["w"], b + lowrank.densify(msg)["w"])
    assert torch.equal(lowrank.apply_(model, {"w": b, "new": 5})["w"], b) and model["new"] == 5
    assert np.array_equal(lowrank.apply_({"w": b.clone()}, msg)["steps"].numpy(), [7])
