"""Low-rank updates on the host (no GPU): compress against torch.linalg.svd, the pickle and ingest round trips,
lowrank_route's three outcomes and plan_lowrank's tables for ragged ranks."""
import pickle

import numpy as np
import pytest
import torch

from flame_amd import _native as N
from flame_amd import engine, ingest, lowrank

G = torch.Generator().manual_seed(0)
DELTA = {"w": torch.randn(40, 24, generator=G), "conv": torch.randn(6, 4, 3, 3, generator=G), "h": torch.randn(9, 30, generator=G).bfloat16(),
         "b": torch.randn(50, generator=G), "n": torch.tensor(4)}


@pytest.mark.parametrize("rank", [1, 5, 64])
def test_compress_densify_and_the_svd_tail(rank):
    """At full rank densify gives the key back; truncated, the Frobenius error is the tail of torch.linalg.svd's singular values."""
    sent = lowrank.compress(DELTA, rank=rank, min_numel=100)
    assert set(sent.right) == {"w", "conv", "h"} and sent["b"] is DELTA["b"] and sent["n"] is DELTA["n"] and sent.shapes["conv"] == (6, 4, 3, 3)
    for k, (m, n) in {"w": (40, 24), "conv": (6, 36), "h": (9, 30)}.items():
        r, s = min(rank, m, n), torch.linalg.svd(DELTA[k].float().reshape(m, n), full_matrices=False).S
        err = torch.linalg.norm(DELTA[k].float() - lowrank.densify(sent)[k])
        assert sent[k].shape == (m, r) and sent.right[k].shape == (r, n) and abs(float(err) - float(s[r:].square().sum().sqrt())) <= 1e-4 * float(s[0])


def test_pickle_ingest_and_to_round_trips():
    sent = lowrank.compress(DELTA, rank=3, dtype=torch.bfloat16)
    for back in (pickle.loads(pickle.dumps(sent)), ingest.loads(pickle.dumps({"weights": sent}))["weights"]):
        assert type(back) is lowrank.LowRankWeights and back.shapes == sent.shapes and list(back) == list(sent) and all(
            torch.equal(back[k], sent[k]) and (k not in sent.right or torch.equal(back.right[k], sent.right[k])) for k in sent)


def test_route_true_false_and_typeerror():
    agg = {k: v.float() for k, v in DELTA.items()}
    ws = [lowrank.compress(agg, rank=r) for r in (2, 5)]
    assert [engine.lowrank_route(torch.float32, ws, k, agg[k].shape) for k in ("w", "conv", "b")] == [True, True, False]
    with pytest.raises(TypeError, match="factored in update 0 and dense in update 1.*supported"):
        engine.lowrank_route(torch.float32, [ws[0], lowrank.densify(ws[1])], "w", agg["w"].shape)


def test_plan_tables_for_ragged_ranks():
    U, V, rates = 0x10000, 0x20000, [0.5, 0.25, 0.125, 0.1]
    ranks, left, right = [[3, 0, 8, 1], [0, 0, 0, 0]], [[U, U + 0x1000, U + 0x2000, U + 0x3004]] * 2, [[V, V + 0x1000, V + 0x2000, V + 0x3000]] * 2
    meta, n_tiles, n_rows, offs = engine.plan_lowrank([(64, 64, 200, 132), (128, 128, 5, 7)], left, right, ranks, rates, 4, tile=128, stage=16)
    head = meta[offs["segs"] // 8:][:16].reshape(2, N.LOWRANK_SEGMENT_INT64S)
    assert head.tolist() == [[64, 64, 200, 132, 0, 0, 16, 0], [128, 128, 5, 7, 4, 16, 0, 0]] and (n_tiles, n_rows) == (5, 16)
    rows = meta[offs["rows"] // 8:][:16 * N.LOWRANK_ROW_INT64S].view(engine.LOWRANK_ROW)
    owner = [0, 0, 0, None, 2, 2, 2, 2, 2, 2, 2, 2, 3, None, None, None]           # client 1 (rank 0) has no row; odd ranks are padded
    q = [0, 1, 2, 0, 0, 1, 2, 3, 4, 5, 6, 7, 0, 0, 0, 0]
    want = [(0, 0, 0, 0.0) if c is None else (left[0][c] + 4 * j, right[0][c] + 4 * 132 * j, ranks[0][c], float(np.float32(rates[c]))) for c, j in zip(owner, q)]
    assert list(zip(*(rows[f].tolist() for f in ("u", "v", "ld", "rate")))) == want
    UV, VV = N.FLAME_LOWRANK_ROW_UVEC, N.FLAME_LOWRANK_ROW_VVEC      # quads 1 and 2 are client 2's columns 0-3 and 4-7; 132 % 4 == 0
    assert rows["flags"].tolist() == [VV, VV, VV, 0, UV | VV, VV, VV, VV, UV | VV, VV, VV, VV, VV, 0, 0, 0]
    with pytest.raises(ValueError, match="plan_lowrank"):
        engine.plan_lowrank([(64, 64, 5, 5)], left[:1], right[:1], [[1, -2, 0, 0]], rates, 4, tile=128, stage=16)


def test_ragged_key_sets_are_one_launch_per_group_and_factor_dtype():
    """Updates 0, 2 and 3 hold w (fp32 factors); all five hold u (bf16) and x (fp32): group (0, 2, 3) is one launch, group (0..4)
    one per factor dtype in first-seen order, each over its own clients' rows and rates (the recorders of
    tests/test_engine_launch_trace.py stand in for the library)."""
    import uplink_cases as UC
    from test_engine_launch_trace import CPU, STREAM
    from test_uplink16_host import _calls, traced
    shapes, carriers = {"w": (129, 127), "u": (31, 33), "x": (32, 32)}, {"w": (0, 2, 3)}
    base, ups = UC.lowrank_case({"w": torch.float32, "u": torch.bfloat16, "x": torch.float32}, shapes=shapes, carriers=carriers)
    agg, rates = {k: torch.from_numpy(v) for k, v in base.items()}, UC.rates_of(5)
    ws = [UC.lowrank_weights(up, shapes) for up in ups]
    with traced(lowrank_tile=lambda: 128, lowrank_stage_rows=lambda: 16) as tr:
        engine.accumulate(agg, list(zip(ws, rates)), device=CPU)
    calls = _calls(tr)
    assert [c[0] for c in calls] == ["flame_agg_reduce_lowrank"] * 3
    for (_, a), key, cis, code, tiles in zip(calls, "wux", (carriers["w"], range(5), range(5)), (N.FLAME_F32, N.FLAME_BF16, N.FLAME_F32), (2, 1, 1)):
        ranks = [ws[c][key].shape[1] for c in cis]
        k_rows = -(-sum(r + (r & 1) for r in ranks) // 16) * 16
        assert a[:3] == [N.FLAME_F32, code, 0] and a[4:6] == [1, tiles] and a[7:] == [k_rows, STREAM]
        words = tr.blocks[a[3]["block"]].numpy()
        assert words[:N.LOWRANK_SEGMENT_INT64S].tolist() == [agg[key].data_ptr(), agg[key].data_ptr(), *shapes[key], 0, 0, k_rows, 0]
        rows = words[a[6]["off"] // 8:][:k_rows * N.LOWRANK_ROW_INT64S].view(engine.LOWRANK_ROW)
        real = rows[rows["u"] != 0]
        want = [(ws[c][key].data_ptr() + q * ws[c][key].element_size(), float(np.float32(rates[c]))) for c, r in zip(cis, ranks) for q in range(r)]
        assert list(zip(real["u"].tolist(), real["rate"].tolist())) == want, key
