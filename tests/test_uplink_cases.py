"""The case builders of tests/uplink_cases.py against independent evaluations (no GPU): a torch fp32 loop over sparse.densify,
lowrank.densify in fp64, a plain Python loop for the bad-index rule; and the structure the GPU tests rely on."""
import numpy as np
import pytest
import torch

import lowrank_ref
import uplink_cases as UC
from flame_amd import lowrank, sparse


def _dense_loop(base, ws, rates):
    """acc = f32(acc + f32(v * rate)) over densify(update), client by client, where the update holds an entry (torch fp32, CPU)."""
    acc = torch.from_numpy(np.array(base, dtype=np.float32)).reshape(-1)
    for w, r, k in ws:
        held = torch.zeros(acc.numel(), dtype=torch.bool)
        held[w.indices[k].long()] = True
        acc = torch.where(held, acc + sparse.densify(w)[k].reshape(-1) * torch.tensor(r, dtype=torch.float32), acc)
    return acc


def _same(label, got, want):
    g, w = got.reshape(-1), want.reshape(-1)
    nan = torch.isnan(g) & torch.isnan(w)
    assert bool((nan | (g.view(torch.int32) == w.view(torch.int32))).all()), label


@pytest.mark.parametrize("numels", [UC.NUMELS, {**UC.NUMELS, "z": 0}, {"a": 1, "b": 1023, "e": 4097, "f": 3 * 4096 + 5}], ids=["plain", "z", "late"])
def test_sparse_case_and_its_reference(numels):
    base, ups = UC.sparse_case(9, numels)
    rates = UC.rates_of(9)
    ws = [UC.sparse_weights(u, numels) for u in ups]
    want = UC.sparse_want(base, ups, rates)
    for k, m in numels.items():
        assert all(u[k][0].dtype == np.int32 and UC.bad_count(u[k][0], m) == 0 for u in ups), k
        assert want[k].shape == (m,) and not any(UC.SPARE in u[k][0] for u in ups)
        _same(k, _dense_loop(base[k], [(w, r, k) for w, r in zip(ws, rates)], rates), want[k])
    assert all(u[k][0].size == 0 for k, u in ((k, ups[3]) for k in numels))         # the client without entries
    assert "z" not in numels or all(u["z"][0].size == 0 for u in ups)


def test_sparse_group_case():
    model, ups = UC.sparse_group_case()
    assert [sorted(u) for u in ups] == [["b", "n", "v", "w"] if c in UC.V_CARRIERS else ["b", "n", "w"] for c in range(6)]
    assert all(sorted(u.indices) == (["v", "w"] if c in UC.V_CARRIERS else ["w"]) for c, u in enumerate(ups))
    assert model["n"].dim() == 0 and model["n"].dtype == torch.int64 and abs(sum(UC.GROUP_RATES) - 1) < 1e-12
    want = UC.sparse_want({k: model[k].numpy() for k in "wv"}, UC.as_numpy(ups, "wv"), UC.GROUP_RATES)
    for k in "wv":
        held = [(u, r, k) for u, r in zip(ups, UC.GROUP_RATES) if k in u]
        assert len(held) == (3 if k == "v" else 6) and all(UC.bad_count(u.indices[k].numpy(), model[k].numel()) == 0 for u, _, _ in held)
        _same(k, _dense_loop(model[k].numpy(), held, None), want[k])
    _, bad = UC.sparse_group_case(bad=True)
    counts = {(c, k): UC.bad_count(u.indices[k].numpy(), model[k].numel()) for c, u in enumerate(bad) for k in u.indices}
    assert {ck: n for ck, n in counts.items() if n} == {(3, "v"): 1} and UC.V_CARRIERS.index(3) == 1      # entry position 3, in-group 1


def _loop_count(idx, numel):
    n = 0
    for p, v in enumerate(idx):
        v = int(v)
        if v < 0 or v >= numel or (p > 0 and v <= int(idx[p - 1])):
            n += 1
    return n


def test_bad_index_rule_and_the_planted_positions():
    rng = np.random.default_rng(0)
    for _ in range(50):         # the numpy rule against the loop, over arrays that hold every kind of bad entry
        numel = int(rng.integers(1, 60))
        idx = rng.choice([UC.I32_MIN, -1, 0, numel - 1, numel, UC.I32_MAX, *rng.integers(0, numel, 6)], int(rng.integers(0, 40))).astype(np.int32)
        assert UC.bad_count(idx, numel) == _loop_count(idx, numel)
    _, good = UC.wide_case(False)
    _, bad = UC.wide_case(True)
    assert UC.WIDE_PER == -(-UC.WIDE_NNZ // -(-UC.WIDE["p"] // 4096)) == 75            # per = ceil(nnz / seg_chunks)
    for c in range(3):
        p = good[c]["p"][0]
        assert p.size == UC.WIDE_NNZ and all(_loop_count(good[c][k][0], m) == 0 for k, m in UC.WIDE.items())
        assert (p[0], p[-1]) == (0, UC.WIDE["p"] - 1) and all(p[j] + 1 == p[j + 1] for j in (74, 149, 224)) and (p[74], p[75]) == (3000, 3001)
        assert (p[149], p[150]) == (4095, 4096)        # two slices meet on the chunk seam
    kinds = {kind for kind, _ in UC.PLANTED_P.values()} | {kind for kind, _ in UC.PLANTED_Q.values()}
    assert kinds == {"duplicate", "descending", "negative", ">= numel", "INT32_MIN", "INT32_MAX"}
    assert sorted(UC.PLANTED_P) == [0, 63, 64, 74, 75, 299]      # first, the lane wrap, a slice end and the next slice's start, last
    for c, key, planted in ((1, "p", UC.PLANTED_P), (2, "q", UC.PLANTED_Q)):
        g, b = good[c][key][0].astype(np.int64), bad[c][key][0].astype(np.int64)
        assert np.flatnonzero(g != b).tolist() == sorted(planted) and np.array_equal(good[c][key][1], bad[c][key][1])
        assert [int(b[pos]) for pos in sorted(planted)] == [int(planted[pos][1](g, UC.WIDE[key])) for pos in sorted(planted)]
    counts = [[_loop_count(u[k][0], m) for k, m in UC.WIDE.items()] for u in bad]
    assert counts == [[0, 0], [6, 0], [0, 2]] and [UC.bad_count(u[k][0], m) for u in bad for k, m in UC.WIDE.items()] == sum(counts, [])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
def test_lowrank_case_and_its_reference(dtype, integer):
    """lowrank.densify in fp64 agrees with tests/lowrank_ref.py within the bound the GPU tests use: both are fp64 sums of the same
    products up to the fp32 rounding of U * rate, which the bound's mag covers (one of its K + 1 roundings)."""
    base, ups = UC.lowrank_case(dtype, integer)
    rates = UC.POW2_RATES if integer else UC.rates_of(5)
    for ki, k in enumerate(UC.LR_SHAPES):
        ranks = [up[k][0].shape[1] for up in ups]
        assert ranks == [UC.LR_RANKS[(c + ki) % 5] for c in range(5)] and 0 in ranks and any(r % 2 for r in ranks)
        assert all(up[k][0].dtype == dtype and up[k][0].shape[0] == UC.LR_SHAPES[k][0] and up[k][1].shape == (r, UC.LR_SHAPES[k][1]) for up, r in zip(ups, ranks))
        dense = torch.from_numpy(base[k]).double()
        for up, r in zip(ups, rates):
            w = lowrank.LowRankWeights({k: up[k][0].double()}, {k: up[k][1].double()}, {k: UC.LR_SHAPES[k]})
            dense = dense + r * lowrank.densify(w)[k].double()          # (densify multiplies in fp32: the factors go in as fp64)
        exact, mag = lowrank_ref.accumulate(base[k], [tuple(f.float().numpy() for f in up[k]) for up in ups], rates)
        assert (np.abs(dense.numpy() - exact) <= lowrank_ref.gamma(sum(ranks) + 1) * mag).all(), k
        if integer:
            assert np.array_equal(dense.numpy(), exact) and np.array_equal(exact, exact.astype(np.float32))      # exact in fp32: the bitwise case
    UC.lowrank_check("the reference itself", {k: torch.from_numpy(lowrank_ref.accumulate(base[k], [tuple(f.float().numpy() for f in up[k]) for up in ups], rates)[0].astype(np.float32))
                                              for k in base}, base, ups, rates, bitwise=integer)


def test_snapshot_sees_a_write_a_move_and_a_restride():
    ts = [torch.arange(6.0).reshape(2, 3), torch.arange(6.0).reshape(3, 2).t(), torch.empty(0), torch.ones(4, dtype=torch.bfloat16)]
    snap = UC.snapshot(ts)
    UC.assert_unchanged("as it was", snap)
    ts[1][0, 1] = 9.0
    with pytest.raises(AssertionError, match="tensor 1 was written"):
        UC.assert_unchanged("written", snap)
    UC.assert_unchanged("bytes not compared", snap, bytes_too=False)
    ts[3].resize_(2, 2)
    with pytest.raises(AssertionError, match="tensor 3 moved or was reshaped"):
        UC.assert_unchanged("reshaped", snap, bytes_too=False)


def test_lowrank_ragged_key_sets():
    carriers = {"w": (0, 2, 3)}
    base, ups = UC.lowrank_case({"w": torch.float32, "u": torch.bfloat16, "x": torch.float32}, shapes={"w": (129, 127), "u": (31, 33), "x": (32, 32)}, carriers=carriers)
    assert [sorted(up) for up in ups] == [["u", "w", "x"] if c in carriers["w"] else ["u", "x"] for c in range(5)]
    assert {up["u"][0].dtype for up in ups} == {torch.bfloat16} and {up["x"][1].dtype for up in ups} == {torch.float32}
    assert [ups[c]["w"][0].shape[1] for c in carriers["w"]] == [0, 3, 8]       # the group's ranks: a 0, an odd one
