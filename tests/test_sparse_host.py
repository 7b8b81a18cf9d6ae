"""Sparse updates on the host (no GPU): the format, every refusal (a TypeError naming sparse updates, nothing
launched) and the two-launch trace of engine.accumulate under tests/test_engine_launch_trace.py's recorders."""
import pickle

import numpy as np
import pytest
import torch

from flame_amd import engine, sparse
from flame_amd.optimizers import optimizer_provider

import uplink_cases as UC
from test_engine_launch_trace import CPU, STREAM
from test_mx_host import _cache
from test_uplink16_host import _calls, traced

NUMELS = {"a": 1, "b": 4097, "c": 2 * 4096 + 37}
RATES = [0.5, 0.25, 0.125, 0.0625, 0.0625]
SIZES = {"sparse_chunk_elems": lambda: 4096, "sparse_scratch_bytes": lambda n_chunks, n: n_chunks * 4 * n * 8}    # no library there


def _model(dtype=torch.float32):
    return {k: torch.full((n,), 0.5, dtype=dtype) for k, n in NUMELS.items()}


def _updates(agg, n=3):
    g = torch.Generator().manual_seed(1)
    return [(sparse.topk({k: torch.randn(v.shape, generator=g).to(v.dtype) for k, v in agg.items()}), RATES[i]) for i in range(n)]


def _refused(fn, *match):
    with traced(**SIZES) as tr:
        with pytest.raises(TypeError) as e:
            fn()
        assert not _calls(tr), _calls(tr)             # nothing was launched
    assert "sparse update" in str(e.value).lower() and "supported" in str(e.value) and all(m in str(e.value) for m in match), e.value


def test_topk_densify_pickle_and_the_int32_limit():
    g = torch.Generator().manual_seed(0)
    delta = {"w": torch.randn(7, 300, generator=g), "h": torch.randn(50, generator=g).to(torch.bfloat16), "n": torch.tensor(4)}
    sent = sparse.topk(delta, ratio=0.01, min_numel=4)
    assert set(sent.indices) == {"w", "h"} and sent["n"] is delta["n"] and sent.shapes == {"w": (7, 300), "h": (50,)}
    for k, nnz in (("w", 21), ("h", 1)):
        i, flat = sent.indices[k].long(), delta[k].reshape(-1).float()
        assert sent[k].dtype == torch.float32 and sent.indices[k].dtype == torch.int32 and i.shape == (nnz,) and bool((i[1:] > i[:-1]).all())
        assert torch.equal(sent[k], flat[i]) and sent[k].abs().min() >= flat.abs().kthvalue(flat.numel() - nnz + 1).values
    assert bool(((delta["w"] - sparse.densify(sent)["w"]).reshape(-1) == 0).sum() == 21)      # the residual lost what was sent
    assert torch.equal(sparse.densify(sparse.topk({"w": delta["w"]}, ratio=1.0))["w"], delta["w"])
    for back in (pickle.loads(pickle.dumps(sent)), sent.to("cpu")):
        assert type(back) is sparse.SparseWeights and back.shapes == sent.shapes and list(back) == list(sent) and all(
            torch.equal(back[k], sent[k]) and (k not in sent.indices or torch.equal(back.indices[k], sent.indices[k])) for k in sent)
    with pytest.raises(ValueError, match="int32 indices"):
        sparse.topk({"w": torch.empty(2 ** 31, device="meta")})


def test_every_refusal_leaves_the_aggregate_untouched():
    agg = _model()

    def acc(mutate, a=agg):
        entries = _updates(a)
        mutate(entries)
        return lambda: engine.accumulate(a, entries, device=CPU)
    _refused(acc(lambda e: e.__setitem__(1, (sparse.densify(e[1][0]), 0.25))), "'a'", "sparse in update 0 and dense in update 1")
    _refused(acc(lambda e: None, _model(torch.bfloat16)), "torch.bfloat16 aggregate")
    _refused(acc(lambda e: e[2][0].__setitem__("b", e[2][0]["b"].double())), "'b'", "torch.float64", "not 1-D torch.float32")
    for mutate, what in ((lambda i: i.long(), "torch.int64"), (lambda i: i[:-1], "(40,), not torch.int32 (41,)"),
                         (lambda i: i.reshape(1, -1), "(1, 41)")):
        _refused(acc(lambda e: e[0][0].indices.__setitem__("b", mutate(e[0][0].indices["b"]))), "'b'", what)
    _refused(acc(lambda e: e[1][0].shapes.pop("c")), "'c'", "without a SparseWeights.shapes entry")
    _refused(acc(lambda e: e[1][0].shapes.__setitem__("c", (37, 2 * 4096))), "'c'", "is not the aggregate's")
    # the reach: engine.refuse_mx, whose call sites tests/test_mx_host.py pins one by one, ends in refuse_sparse (three of
    # them below); defer=True and the FedOPT family are sites of their own
    ws = [w for w, _ in _updates(agg, n=5)]

    fedopt, get = optimizer_provider.get("fedadam"), optimizer_provider.get
    fedopt.current_weights = {k: torch.zeros_like(v) for k, v in agg.items()}      # past round 1
    do = lambda opt: lambda: opt.do(agg, _cache(ws), total=15, version=1)      # noqa: E731
    for fn, what in ((lambda: engine.refuse_mx(ws, "SCAFFOLD"), "SCAFFOLD does not take sparse updates"), (do(get("fedavg", defer=True)), "defer=True"),
                     (do(fedopt), "FedOPT"), (do(get("fedyogi", defer=True)), "FedOPT"), (do(get("fedbuff")), "FedBuff"),
                     (lambda: engine.accumulate(agg, _updates(agg), device=CPU, key_groups=[["a"], ["b", "c"]]), "sharded wrapper")):
        _refused(fn, what)
    assert all(bool((v == 0.5).all()) for v in agg.values())


@pytest.mark.parametrize("scaled", [False, True])
def test_accumulate_is_an_index_launch_and_a_reduce_launch(scaled):
    agg = _model()
    agg["nbt"] = torch.full((1,), 3)
    entries, scales = _updates(agg), [1.0, 0.5, 0.25] if scaled else None
    with traced(**SIZES) as tr:
        engine.accumulate(agg, entries, device=CPU, scales=scales)
    calls = _calls(tr)
    assert [c[0] for c in calls] == ["flame_sparse_index", "flame_agg_reduce_sparse", "flame_agg_reduce"], [c[0] for c in calls]
    ix, rd, n_chunks, sbytes = calls[0][1], calls[1][1], 1 + 2 + 3, (1 + 2 + 3) * 4 * 3 * 8
    assert ix[1:3] == [3, n_chunks] and ix[5] == 3 and ix[8:] == [sbytes, STREAM]
    assert rd[:2] == [engine.N.FLAME_F32, 0] and rd[3:5] == [3, n_chunks] and rd[8] == 3 and rd[12:] == [sbytes, STREAM]
    assert rd[2] == ix[0] and rd[5] == ix[3] and rd[7] == ix[4] and rd[11] == ix[7]       # one block, one bounds buffer
    words = tr.blocks[ix[0]["block"]].numpy()
    segs = words[:3 * engine.SEG_WORDS].reshape(3, engine.SEG_WORDS)
    assert segs[:, 6].tolist() == list(NUMELS.values()) and segs[:, 7].tolist() == [0, 1, 3]      # chunks of 4,096
    table = lambda a: words[a["off"] // 8: a["off"] // 8 + 9].reshape(3, 3).tolist()              # noqa: E731
    assert table(rd[5]) == [[w.indices[k].data_ptr() for w, _ in entries] for k in NUMELS] and table(rd[7]) == [[1] * 3, [41] * 3, [83] * 3]
    assert table(rd[6]) == [[w[k].data_ptr() for w, _ in entries] for k in NUMELS]
    assert words[rd[9]["off"] // 8:].view(np.float32)[:3].tolist() == RATES[:3]
    assert rd[10] is None if not scaled else words[rd[10]["off"] // 8:].view(np.float32)[:3].tolist() == scales
    nnz, elems = 3 * (1 + 41 + 83), sum(NUMELS.values())
    assert [e[1:] for e in tr.events if e[0] == "timed"][:2] == [["flame_sparse_index", 4 * nnz + sbytes],
                                                                 ["flame_agg_reduce_sparse", 8 * nnz + sbytes + 8 * elems]]


# ---------------------------------------------------------------------------- client groups (tests/uplink_cases.py)
def _bad_counts(tr, per_call):
    """The recorder's flame_sparse_index, which also adds ``per_call[i]`` (one count per client of the group) to the ``bad``
    array of its i-th call, as the kernel would: the array is the engine's own CPU tensor here."""
    import ctypes
    record, seen = tr.__getattr__("flame_sparse_index"), []

    def call(*args):
        counts = per_call[len(seen)]
        seen.append(args)
        assert args[5] == len(counts)
        bad = (ctypes.c_int64 * len(counts)).from_address(args[6])
        for i, c in enumerate(counts):
            bad[i] += c
        return record(*args)
    tr.flame_sparse_index = call


def test_key_set_groups_index_every_group_before_reducing_any():
    """Two client groups, (0..5) with w sparse and b, n dense, (1, 3, 4) with v sparse: both index launches, then group by group
    the gather and the group's dense keys (one launch per dtype)."""
    model, ups = UC.sparse_group_case()
    with traced(**SIZES) as tr:
        engine.accumulate(model, list(zip(ups, UC.GROUP_RATES)), device=CPU)
    calls = _calls(tr)
    assert [c[0] for c in calls] == ["flame_sparse_index"] * 2 + ["flame_agg_reduce_sparse", "flame_agg_reduce", "flame_agg_reduce", "flame_agg_reduce_sparse"]
    assert [(c[1][1], c[1][2], c[1][5]) for c in calls[:2]] == [(1, 2, 6), (1, 1, 3)]         # (segments, chunks, clients) per group
    assert calls[2][1][2] == calls[0][1][0] and calls[5][1][2] == calls[1][1][0]              # each gather on its own group's block
    for call, key, cis in ((calls[0], "w", range(6)), (calls[1], "v", UC.V_CARRIERS)):         # the group's own clients and rates
        words, n = tr.blocks[call[1][0]["block"]].numpy(), len(cis)
        table = lambda a: words[a["off"] // 8: a["off"] // 8 + n].tolist()                     # noqa: E731
        assert table(call[1][3]) == [ups[c].indices[key].data_ptr() for c in cis] and table(call[1][4]) == [ups[c][key].numel() for c in cis]
        rd = calls[2 if key == "w" else 5][1]
        assert words[rd[9]["off"] // 8:].view(np.float32)[:n].tolist() == [float(np.float32(UC.GROUP_RATES[c])) for c in cis]


def test_a_bad_index_in_a_later_group_names_the_entry_position():
    """The second group's index launch reports one bad entry for its client 1, which is update 3 of the call: the message says 3,
    and no reduction of either group has been launched."""
    model, ups = UC.sparse_group_case(bad=True)
    with traced(**SIZES) as tr:
        _bad_counts(tr, [[0] * 6, [UC.bad_count(ups[c].indices["v"].numpy(), 1025) for c in UC.V_CARRIERS]])
        with pytest.raises(ValueError, match=r"position\(s\) 3 \(1 bad entries\) hold"):
            engine.accumulate(model, list(zip(ups, UC.GROUP_RATES)), device=CPU)
    assert [c[0] for c in _calls(tr)] == ["flame_sparse_index"] * 2
    with traced(**SIZES) as tr:          # several clients of several groups: every group is checked in order, the first bad one raises
        _bad_counts(tr, [[0, 0, 2, 0, 0, 7], [4, 0, 0]])
        with pytest.raises(ValueError, match=r"position\(s\) 2 \(2 bad entries\), 5 \(7 bad entries\) hold"):
            engine.accumulate(model, list(zip(ups, UC.GROUP_RATES)), device=CPU)
    assert [c[0] for c in _calls(tr)] == ["flame_sparse_index"] * 2


def test_a_key_sparse_in_one_update_and_factored_in_another_is_refused():
    """sparse_route sees the low-rank update as "dense": the message names the key and both updates, whichever comes first."""
    from flame_amd import lowrank
    agg = {"w": torch.full((40, 50), 0.5), "b": torch.full((7,), 0.5)}
    sp = sparse.topk({"w": torch.ones(40, 50), "b": torch.ones(7)}, min_numel=8)
    lr = lowrank.compress({"w": torch.ones(40, 50), "b": torch.ones(7)}, rank=2)
    for entries, what in (([(sp, 0.5), (lr, 0.5)], "sparse in update 0 and dense in update 1"), ([(lr, 0.5), (sp, 0.25), (sp, 0.25)], "sparse in update 1 and dense in update 0")):
        _refused(lambda: engine.accumulate(agg, entries, device=CPU), "'w'", what, "per-key mixtures of sparse and dense updates are not supported")
    assert all(bool((v == 0.5).all()) for v in agg.values())
