"""flame_sparse_index + flame_agg_reduce_sparse on the GPU, BITWISE against tests/sparse_ref.py: the shapes,
entry counts, edges and values at which the gather can go wrong; the bad-index refusals; the densified equivalence.  Then what
lies between engine.accumulate and the launches: host-resident updates and aggregates, late inputs on a stream of their own, client
groups with different key sets, validation past one lane and one slice, and the out-of-place and empty-segment branches of the two
C entry points, which the engine never takes (case builders: tests/uplink_cases.py)."""
import numpy as np
import pytest
import torch

import scenarios as S
import sparse_ref
import stream_case as SC
import uplink_cases as UC
from large_case import Launches
from test_mx_host import _cache

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
NUMELS, _case = UC.NUMELS, UC.sparse_case        # the arithmetic case: tests/uplink_cases.py


def _dev(a, misalign=False):     # a on the device; misalign: as a view 4 bytes into its buffer (4-byte, not 16-byte aligned)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    buf[1:] = torch.from_numpy(a)
    return buf[1:] if misalign else buf[1:].clone()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", [1, 8, 9, 70])
def test_reduce_matches_the_contract(n, scaled):
    """Odd clients' index and value tensors are misaligned views; at n = 9 the aggregate is one too (FLAME_SEG_UNALIGNED)."""
    from flame_amd import engine, sparse
    base, ups = _case(n)
    rates = [(c + 1) / (n * (n + 1) / 2) for c in range(n)]
    scales = [1.0 if c % 3 else 1.0 / (c + 3) for c in range(n)] if scaled else None
    want = {k: torch.from_numpy(sparse_ref.accumulate(base[k], [u[k] for u in ups], rates, scales)) for k in base}
    ws = [sparse.SparseWeights({k: _dev(v, c % 2) for k, (_, v) in u.items()}, {k: _dev(i, c % 2) for k, (i, _) in u.items()},
                               {k: (NUMELS[k],) for k in u}) for c, u in enumerate(ups)]
    got = []
    for _ in range(2):
        agg = {k: _dev(v, n == 9) for k, v in base.items()}
        with Launches() as ln:
            engine.accumulate(agg, list(zip(ws, rates)), scales=scales)
        assert ln.names == ["flame_sparse_index", "flame_agg_reduce_sparse"], ln.names
        S.same_bits(f"sparse n={n}", agg, want)
        got.append(agg)
    assert all(torch.equal(got[0][k].view(torch.int32), got[1][k].view(torch.int32)) for k in base)      # equal launches, equal bits


@pytest.mark.parametrize("idx", [[3, 9, 8, 20], [3, 9, 9, 20], [-1, 9, 10, 20], [3, 9, 10, 5000]], ids=["unsorted", "duplicate", "negative", "numel"])
def test_bad_indices_raise_before_the_reduce(idx):
    from flame_amd import engine, sparse
    agg = {"w": torch.ones(5000, device=DEV), "d": torch.ones(9, device=DEV)}
    good, bad = (sparse.SparseWeights({"w": torch.ones(4), "d": torch.ones(9)}, {"w": torch.tensor(i, dtype=torch.int32)},
                                      {"w": (5000,)}).to(DEV) for i in ([0, 1, 2, 4999], idx))
    with Launches() as ln:
        with pytest.raises(ValueError, match=r"position\(s\) 1 \(1 bad entries\)"):
            engine.accumulate(agg, [(good, 0.5), (bad, 0.25), (good, 0.25)])
    assert ln.names == ["flame_sparse_index"] and all(bool((v == 1).all()) for v in agg.values()), ln.names


@pytest.mark.parametrize("sort,noise", [("accumulate", None), ("fedavg", None), ("fedavg", 0.01), ("fedprox", None), ("fedprox", 0.01)])
def test_equals_the_round_over_the_densified_updates(sort, noise):
    from flame_amd import engine, sparse
    from flame_amd.optimizers import optimizer_provider
    g = torch.Generator().manual_seed(11)
    model = {"w": torch.randn(3, 4099, generator=g), "b": torch.randn(77, generator=g), "n": torch.tensor(3)}
    ups = [sparse.topk({k: torch.randn(v.shape, generator=g).to(v.dtype) for k, v in model.items()}, ratio=0.03) for _ in range(4)]
    out = []
    for dense in (False, True):
        ws = [{k: v.to(DEV) for k, v in sparse.densify(u).items()} if dense else u.to(DEV) for u in ups]
        agg, cache = {k: v.to(DEV) for k, v in model.items()}, S.SortedCache()
        for i, w in enumerate(ws):
            cache[f"e{i}"] = S.TR(w, 2 + i, 0)
        if sort == "accumulate":
            engine.accumulate(agg, [(w, (2 + i) / 14) for i, w in enumerate(ws)])
        else:
            kw = {"mu": 0.1} if sort == "fedprox" else {}
            agg = optimizer_provider.get(sort, **kw, **({} if noise is None else {"noise_factor": noise, "noise_seed": 9})).do(agg, cache, total=14)
        out.append(agg)
    S.same_bits(f"{sort} sparse vs densify", out[0], {k: v.cpu() for k, v in out[1].items()})


# ---------------------------------------------------------------------------- residency: engine._staged, engine._Target
WITH_Z = {**NUMELS, "z": 0}
_CASE9 = {}


def _case9(numels):     # (base, ups, rates, want), computed once per key set and never written
    if tuple(numels) not in _CASE9:
        base, ups = _case(9, numels)
        _CASE9[tuple(numels)] = (base, ups, UC.rates_of(9), UC.sparse_want(base, ups, UC.rates_of(9)))
    return _CASE9[tuple(numels)]


@pytest.mark.parametrize("agg_where", ["gpu", "pageable"])
@pytest.mark.parametrize("where", ["gpu", "pinned", "pageable"])
def test_residency(where, agg_where):
    """Indices and values on ``where``, the fp32 aggregate on ``agg_where``: host updates are copied by engine._staged, a host aggregate
    goes through engine._Target and its write-back.  n = 9 is one unrolled step of 8 clients and the remainder loop; key z has no element."""
    from flame_amd import engine
    base, ups, rates, want = _case9(WITH_Z)
    ws = [UC.sparse_weights(u, WITH_Z, lambda a: UC.place(a, where)) for u in ups]
    agg = {k: UC.place(v, agg_where) for k, v in base.items()}
    read, held, objs = UC.snapshot([t for w in ws for t in (*w.values(), *w.indices.values())]), UC.snapshot(agg.values()), dict(agg)
    with Launches() as ln:
        engine.accumulate(agg, list(zip(ws, rates)))
    torch.cuda.synchronize()
    assert ln.names == ["flame_sparse_index", "flame_agg_reduce_sparse"], ln.names
    S.same_bits(f"sparse {where} into {agg_where}", agg, want)
    UC.assert_unchanged("updates", read)
    UC.assert_unchanged("aggregate", held, bytes_too=False)
    assert all(agg[k] is objs[k] and agg[k].is_cuda == (agg_where == "gpu") for k in objs)


# ---------------------------------------------------------------------------- the stream contract
LATE = {k: NUMELS[k] for k in "abef"}
SYNC = "_SparseRound.check reads the counters back"


@pytest.fixture(scope="module")
def delay():
    d = SC.Delay()
    yield d
    d.free()


def _late_weights(late, ups, where, group):
    return [UC.sparse_weights(u, LATE, lambda a: late.tensor(torch.from_numpy(a.copy()), where, group)) for u in ups]


@pytest.mark.parametrize("where", ["gpu", "pinned"])
def test_late_inputs_on_a_stream_of_their_own(delay, where):
    """Every index, value and aggregate buffer holds poison (-7: as an index, a bad one) until a delay on the test's stream has run:
    an index launch that does not wait raises ValueError.  The gather is launched after check() has waited for the stream, so it
    cannot be early; it can only be unordered against what FOLLOWS on the stream.  So the update tensors are then dropped, their
    blocks re-poisoned on the stream, and a second round (the clients in reverse) goes into the same aggregate: that sees a gather
    still pending elsewhere only sometimes (tests/stream_case.py, step 7)."""
    from flame_amd import engine
    base, ups, rates, want0 = _case9(LATE)
    want = [want0, UC.sparse_want({k: v.numpy() for k, v in want0.items()}, ups[::-1], rates)]

    def case(late):
        agg = late.weights({k: torch.from_numpy(v) for k, v in base.items()})
        ws = [_late_weights(late, r, where, g) for g, r in enumerate((ups, ups[::-1]))]
        res = {}
        with late.stream():
            for g in (0, 1):
                late.start(g)
                with late.call(f"sparse accumulate, round {g}", sync=SYNC):
                    engine.accumulate(agg, list(zip(ws[g], rates)))
                res[f"round{g}"] = late.snap(agg)
                late.reuse(*[d for w in ws[g] for d in (w, w.indices)])
        late.finish()
        for g in (0, 1):
            S.same_bits(f"late={not late.ready} round {g}", res[f"round{g}"], want[g])
        return {k: SC.cpu(v) for k, v in res.items()}
    ready = case(SC.Late(delay, ready=True))
    SC.assert_same("sparse", ready, case(SC.Late(delay)))


def test_fedavg_round_on_a_late_stream(delay):
    from flame_amd.optimizers import optimizer_provider
    base, ups, rates, want = _case9(LATE)          # rates_of(9) are counts 1..9 over their total of 45

    def case(late):
        agg = late.weights({k: torch.from_numpy(v) for k, v in base.items()})
        ws = _late_weights(late, ups, "gpu", 0)
        with late.stream():
            late.start()
            with late.call("sparse fedavg", sync=SYNC):
                out = optimizer_provider.get("fedavg").do(agg, _cache(ws, list(range(1, 10))), total=45)
            res = late.snap(out)
        late.finish()
        assert out is agg
        S.same_bits(f"late={not late.ready}", res, want)
        return {"out": SC.cpu(res)}
    ready = case(SC.Late(delay, ready=True))
    SC.assert_same("sparse fedavg", ready, case(SC.Late(delay)))


# ---------------------------------------------------------------------------- client groups (tests/uplink_cases.py)
def _group_case(bad=False):
    model, ups = UC.sparse_group_case(bad)
    return model, ups, {k: v.to(DEV) for k, v in model.items()}, [u.to(DEV) for u in ups]


def test_key_set_groups():
    """w is sparse in all six updates, v in updates 1, 3 and 4 only; b and n are dense: both groups are indexed, then each group is
    reduced (its gather, then its dense keys, one launch per dtype).  w and v: tests/sparse_ref.py over the group's own clients and
    rates.  b and n: the bits of the round over the dense keys alone."""
    from flame_amd import engine
    model, ups, agg, ws = _group_case()
    with Launches() as ln:
        engine.accumulate(agg, list(zip(ws, UC.GROUP_RATES)))
    assert ln.names == ["flame_sparse_index"] * 2 + ["flame_agg_reduce_sparse", "flame_agg_reduce", "flame_agg_reduce", "flame_agg_reduce_sparse"], ln.names
    S.same_bits("groups", agg, UC.sparse_want({k: model[k].numpy() for k in "wv"}, UC.as_numpy(ups, "wv"), UC.GROUP_RATES))
    dense = {k: model[k].to(DEV) for k in "bn"}
    engine.accumulate(dense, [({k: w[k] for k in "bn"}, r) for w, r in zip(ws, UC.GROUP_RATES)])
    S.same_bits("dense keys", agg, {k: v.cpu() for k, v in dense.items()})
    assert not torch.equal(dense["b"].cpu(), model["b"]) and int(dense["n"]) != int(model["n"])


def test_a_bad_index_in_a_later_group_raises_before_any_group_is_reduced():
    """Update 3 repeats an index of v: it is client 1 of the second group, and the message names position 3."""
    from flame_amd import engine
    model, _, agg, ws = _group_case(bad=True)
    with Launches() as ln:
        with pytest.raises(ValueError, match=r"position\(s\) 3 \(1 bad entries\) hold"):
            engine.accumulate(agg, list(zip(ws, UC.GROUP_RATES)))
    assert ln.names == ["flame_sparse_index"] * 2, ln.names
    S.same_bits("untouched", agg, model)


# ---------------------------------------------------------------------------- validation at width
@pytest.mark.parametrize("bad", [True, False], ids=["planted", "good"])
def test_validation_at_width(bad):
    """300 entries over a key of 4 chunks: 75 positions per slice, so the lane loop runs twice and positions 74 | 75 are read by
    different workgroups.  planted: client 1's first key holds six bad entries (uplink_cases.PLANTED_P), client 2's second key two;
    the counts are the stated rule's (tests/test_uplink_cases.py checks them against a loop).  good: the same arrays unplanted,
    consecutive integers across every slice seam: nothing is counted and the sum is tests/sparse_ref.py's."""
    from flame_amd import engine
    base, ups = UC.wide_case(bad)
    rates = [0.5, 0.25, 0.25]
    agg = {k: _dev(v) for k, v in base.items()}
    ws = [UC.sparse_weights(u, UC.WIDE, _dev) for u in ups]
    counts = [sum(UC.bad_count(u[k][0], m) for k, m in UC.WIDE.items()) for u in ups]
    with Launches() as ln:
        if bad:
            assert counts == [0, 6, 2]
            with pytest.raises(ValueError) as e:
                engine.accumulate(agg, list(zip(ws, rates)))
            assert f"position(s) 1 ({counts[1]} bad entries), 2 ({counts[2]} bad entries) hold" in str(e.value), e.value
        else:
            assert counts == [0, 0, 0]
            engine.accumulate(agg, list(zip(ws, rates)))
    assert ln.names == ["flame_sparse_index"] + ["flame_agg_reduce_sparse"] * (not bad), ln.names
    S.same_bits("width", agg, {k: torch.from_numpy(v) for k, v in base.items()} if bad else UC.sparse_want(base, ups, rates))


# ---------------------------------------------------------------------------- the C entry points, where the engine never goes
def _raw(outs, ins, idx, val, rates, fill=None):
    """flame_sparse_index, then flame_agg_reduce_sparse over ``out != in`` tables of engine.plan_sparse, on the current stream with
    the scratch engine._SparseRound allocates: ``(bad counts, the bounds scratch)`` after a synchronise."""
    from flame_amd import _native as N, engine
    L, n, st = N.lib(), len(rates), torch.cuda.current_stream().cuda_stream
    segs = [engine.Seg(i.numel(), out=o.data_ptr(), inp=i.data_ptr()) for o, i in zip(outs, ins)]
    assert all(o.numel() == i.numel() and len(ri) == len(rv) == n and all(a.numel() == b.numel() for a, b in zip(ri, rv)) for o, i, ri, rv in zip(outs, ins, idx, val))
    meta, n_chunks, o = engine.plan_sparse(segs, [[t.data_ptr() for t in r] for r in idx], [[t.data_ptr() for t in r] for r in val],
                                           [[t.numel() for t in r] for r in idx], rates)
    sbytes = engine.sparse_scratch_bytes(n_chunks, n)
    bounds = torch.empty(sbytes, dtype=torch.uint8, device=DEV) if fill is None else torch.full((sbytes,), fill, dtype=torch.uint8, device=DEV)
    bad, block = torch.zeros(n, dtype=torch.int64, device=DEV), torch.from_numpy(meta).to(DEV)
    b = block.data_ptr()
    N.check(L.flame_sparse_index(b, len(segs), n_chunks, b + o["indices"], b + o["nnz"], n, bad.data_ptr(), bounds.data_ptr(), sbytes, st))
    N.check(L.flame_agg_reduce_sparse(N.FLAME_F32, 0, b, len(segs), n_chunks, b + o["indices"], b + o["values"], b + o["nnz"], n, b + o["r32"], None,
                                      bounds.data_ptr(), sbytes, st))
    torch.cuda.synchronize()
    return bad.cpu().tolist(), bounds.cpu()


def _entries(rng, numel, count, below):      # (int32 indices under ``below``, fp32 values) on the device
    idx = np.sort(rng.choice(min(numel, below), min(count, numel, below), replace=False)).astype(np.int32)
    return idx, (rng.standard_normal(idx.size) * 1e-2).astype(np.float32)


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "unaligned"])
def test_out_of_place_copies_the_ranges_without_entries(misalign):
    """out != in, out full of poison, every entry in sub-range 0 of chunk 0: a wave without an entry must still copy its range
    (the in-place early return is not for it).  out is the reference everywhere, the element either side of it keeps its
    poison, in keeps its bits.  unaligned: both are views one element into their buffers (FLAME_SEG_UNALIGNED)."""
    rng, numels, rates = np.random.default_rng(3), {"d": 1025, "f": 3 * 4096 + 5}, [0.5, 0.25, 0.25]
    base = {k: rng.standard_normal(m).astype(np.float32) for k, m in numels.items()}
    base["f"][5000] = -0.0
    ups = [{k: _entries(rng, m, cnt, 1024) for k, m in numels.items()} for cnt in (5, 64, 70)]
    lo = int(misalign)
    bufs = {k: (torch.full((m + 2,), float(SC.POISON), device=DEV), torch.zeros(m + 2, device=DEV)) for k, m in numels.items()}
    outs, ins = [bufs[k][0][lo:lo + m] for k, m in numels.items()], [bufs[k][1][lo:lo + m] for k, m in numels.items()]
    for t, k in zip(ins, numels):
        t.copy_(torch.from_numpy(base[k]))
    assert all((t.data_ptr() % 16 != 0) == misalign for t in outs + ins)
    bad, _ = _raw(outs, ins, [[_dev(u[k][0]) for u in ups] for k in numels], [[_dev(u[k][1]) for u in ups] for k in numels], rates)
    assert bad == [0, 0, 0]
    S.same_bits("out", dict(zip(numels, outs)), UC.sparse_want(base, ups, rates))
    S.same_bits("in", dict(zip(numels, ins)), {k: torch.from_numpy(v) for k, v in base.items()})
    for k, m in numels.items():
        guard = torch.cat([bufs[k][0][:lo], bufs[k][0][lo + m:]]).cpu()
        assert bool((guard == SC.POISON).all()), f"{k}: written outside out"


def test_launches_of_empty_segments():
    """Only 0-element keys: the launch keeps one idle chunk, whose workgroups return before they touch the scratch.  A 0-element
    key between two others: its neighbours' chunks still find their segments."""
    empty = [torch.empty(0, device=DEV) for _ in range(2)]
    none_i, none_v = [torch.empty(0, dtype=torch.int32, device=DEV)] * 3, [torch.empty(0, device=DEV)] * 3
    bad, bounds = _raw(empty, empty, [none_i] * 2, [none_v] * 2, [0.5, 0.25, 0.25], fill=0xA5)
    assert bad == [0, 0, 0] and bounds.numel() == 4 * 3 * 8 and bool((bounds == 0xA5).all())
    rng, numels, rates = np.random.default_rng(4), {"x": 1025, "z": 0, "y": 4097}, [0.5, 0.25, 0.25]
    base = {k: rng.standard_normal(m).astype(np.float32) for k, m in numels.items()}
    ups = [{k: _entries(rng, m, cnt, m) for k, m in numels.items()} for cnt in (3, 200, 1500)]
    agg = [_dev(base[k]) for k in numels]
    bad, _ = _raw(agg, agg, [[_dev(u[k][0]) for u in ups] for k in numels], [[_dev(u[k][1]) for u in ups] for k in numels], rates)
    assert bad == [0, 0, 0]
    S.same_bits("x z y", dict(zip(numels, agg)), UC.sparse_want(base, ups, rates))
