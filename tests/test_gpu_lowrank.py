"""flame_agg_reduce_lowrank on the GPU against tests/lowrank_ref.py ("the low-rank contract"): the shapes,
ranks, alignments and values at which the tiled product can go wrong; the densified equivalence; the refusals.  Then what lies
between engine.accumulate and the launch: host-resident and strided factors, host aggregates, late inputs on a stream of their
own, ragged key sets with two factor dtypes, sparse, low-rank and dense routes in one call, and the out-of-place branch of the C
entry point, which the engine never takes (case builders: tests/uplink_cases.py)."""
import numpy as np
import pytest
import torch

import lowrank_ref
import scenarios as S
import stream_case as SC
import uplink_cases as UC
from flame_amd import engine, ingest, lowrank, shard, slab
from flame_amd.optimizer import fedbuff, sync_hierarchy
from flame_amd.optimizers import optimizer_provider
from large_case import Launches
from test_mx_host import _cache

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
SHAPES = {"a": (1, 1), "b": (31, 33), "c": (32, 32), "d": (127, 129), "e": (128, 128), "f": (129, 127), "g": (257, 130)}    # the tile is 128
RANKS = (0, 1, 2, 3, 8, 16, 64)


def _case(n, dtype, integer, keys=SHAPES):        # (base {k: fp32 numpy}, ups[c][k] = (U, V) torch CPU tensors of dtype)
    rng = np.random.default_rng(1000 * n + integer)
    draw = (lambda *s: rng.integers(-8, 9, s).astype(np.float32)) if integer else (
        lambda *s: (rng.choice([-1.0, 1.0], s) * 2.0 ** rng.uniform(-10, 10, s)).astype(np.float32))
    ranks = {k: [RANKS[(3 * c + list(SHAPES).index(k) + 1) % 7] for c in range(n)] for k in keys}
    for r in ranks.values():        # a key's sum is never a multiple of the 16-row stage (it is 0 for key g at n = 1)
        r[0] = r[0] if sum(r) % 16 or not sum(r) else 3 if r[0] != 3 else 1
    base = {k: draw(*SHAPES[k]) for k in keys}
    return base, [{k: tuple(torch.from_numpy(draw(*s)).to(dtype) for s in ((SHAPES[k][0], r[c]), (r[c], SHAPES[k][1]))) for k, r in ranks.items()}
                  for c in range(n)]


def _dev(t, misalign=False):     # t on the device; misalign: as a view one element into its buffer (4 / 2 bytes, not 16)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape) if misalign else buf[1:].clone().view(t.shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,kind", [(n, kind) for n in (1, 2, 9, 70) for kind in ("integer", "random")] + [(9, "special")])
def test_reduce_matches_the_contract(n, kind, dtype):
    """Odd clients' factors are misaligned views, at n = 9 the aggregate too.  Every element is non-finite exactly where the fp64
    reference is, else within gamma_{K+1} * mag of it (K = sum r_c), and two launches give equal bits.  integer (power-of-two rates):
    bitwise the reference.  random: magnitudes in [2^-10, 2^10].  special: an inf in a left factor of rank 3, a NaN in a right one of rank 1."""
    base, ups = _case(n, dtype, kind == "integer", keys="f" if kind == "special" else SHAPES)
    if kind == "special":
        assert (ups[6]["f"][0].shape[1], ups[3]["f"][0].shape[1]) == (3, 1)
        ups[6]["f"][0][5, 2], ups[3]["f"][1][0, 7], ups[6]["f"][0][128, 0] = float("inf"), float("nan"), float("-inf")
    rates = [2.0 ** -(c % 5) for c in range(n)] if kind == "integer" else [(c + 1) / (n * (n + 1) / 2) for c in range(n)]
    ws = [lowrank.LowRankWeights({k: _dev(u, c % 2) for k, (u, _) in up.items()}, {k: _dev(v, c % 2) for k, (_, v) in up.items()},
                                 {k: SHAPES[k] for k in up}) for c, up in enumerate(ups)]
    aggs = [{k: _dev(torch.from_numpy(v), n == 9) for k, v in base.items()} for _ in range(2)]
    for agg in aggs:
        with Launches() as ln:
            engine.accumulate(agg, list(zip(ws, rates)))
        assert ln.names == ["flame_agg_reduce_lowrank"], ln.names
    for k, got in aggs[0].items():
        exact, mag = lowrank_ref.accumulate(base[k], [tuple(f.float().numpy() for f in up[k]) for up in ups], rates)
        got64, fin = got.cpu().numpy().astype(np.float64), np.isfinite(exact)
        assert np.array_equal(np.isfinite(got64), fin) and fin.all() == (kind != "special"), f"{k}: non-finite sets differ"
        err, tol = np.abs(got64[fin] - exact[fin]), (lowrank_ref.gamma(sum(up[k][0].shape[1] for up in ups) + 1) * mag)[fin]
        assert (err <= tol).all(), f"{k}: {int((err > tol).sum())} elements outside the bound, worst {np.max(err / np.maximum(tol, 1e-300)):.3g} of it"
        assert torch.equal(got.view(torch.int32), aggs[1][k].view(torch.int32)), k
        if kind == "integer":
            S.same_bits(f"lowrank {k} n={n}", {k: got}, {k: torch.from_numpy(exact.astype(np.float32))})


@pytest.mark.parametrize("sort,noise,where", [("fedavg", None, "device"), ("fedavg", 0.01, "device"), ("fedprox", None, "device"),
                                              ("fedgft", None, "device"), ("fedavg", None, "host"), ("fedavg", None, "stream")])
def test_equals_the_round_over_the_densified_updates(sort, noise, where):
    """Both routes evaluate base + sum rate_c U_c V_c in fp32: K products and at most n + 2 further roundings per element (the
    rate fold, or the dense route's product rounding and scaling).  Each is within gamma_{K+n+2} * mag of the real value, mag =
    |base| + sum rate |U| |V|, so they are within twice that of each other; with noise, one more add of |out|.  Dense keys: bitwise."""
    g = torch.Generator().manual_seed(11)
    model = {"w": torch.randn(150, 131, generator=g), "conv": torch.randn(20, 3, 3, 3, generator=g), "b": torch.randn(77, generator=g), "n": torch.tensor(3)}
    ups = [lowrank.compress({k: torch.randn(v.shape, generator=g).to(v.dtype) for k, v in model.items()}, rank=r) for r in (1, 4, 6, 9)]
    kw = {**{"fedprox": {"mu": 0.1}, "fedgft": {"fair": "SP", "gamma": 0.1}}.get(sort, {}), **({"noise_factor": noise, "noise_seed": 9} if noise else {})}
    out, stream = [], torch.cuda.Stream(DEV) if where == "stream" else torch.cuda.current_stream(DEV)
    for dense in (False, True):
        with torch.cuda.stream(stream):
            ws = [{k: v.to(DEV) for k, v in lowrank.densify(u).items()} if dense else u.to(DEV) for u in ups]
            agg = {k: v.clone() if where == "host" else v.to(DEV) for k, v in model.items()}
            agg = optimizer_provider.get(sort, **kw).do(agg, _cache(ws, [2, 3, 4, 5]), total=14)
        stream.synchronize()
        assert all(v.device.type == ("cpu" if where == "host" else "cuda") for v in agg.values())
        out.append({k: v.cpu() for k, v in agg.items()})
    S.same_bits(f"{sort} dense keys", {k: out[0][k] for k in "bn"}, {k: out[1][k] for k in "bn"})
    for k in ups[0].right:
        mag = model[k].double().abs().flatten(1) + (out[1][k].double().abs().flatten(1) if noise else 0)
        for i, u in enumerate(ups):
            mag += (2 + i) / 14 * (u[k].double().abs() @ u.right[k].double().abs())
        tol = 2 * lowrank_ref.gamma(sum(u[k].shape[1] for u in ups) + len(ups) + 2 + bool(noise)) * mag.reshape(model[k].shape)
        assert bool(((out[0][k].double() - out[1][k].double()).abs() <= tol).all()), k


def _do(agg, ws, name, attrs=(), do_kw=(), **kw):       # optimizer `name`, with attributes set, over the round
    opt = optimizer_provider.get(name, **kw)
    for a, v in dict(attrs).items():
        setattr(opt, a, v)
    return opt.do(agg, _cache(ws), total=15, **dict(do_kw))


# engine.accumulate with update 1 replaced by change(update 1); an update with a factor of "w" replaced; zeros shaped like the model
_acc = lambda agg, ws, change=None, **kw: engine.accumulate(agg, [(change(w) if change and i == 1 else w, 0.2) for i, w in enumerate(ws)], **kw)      # noqa: E731
_with = lambda w, left=None, right=None: type(w)({**w, "w": w["w"] if left is None else left}, {"w": w.right["w"] if right is None else right}, w.shapes)      # noqa: E731
_like = lambda agg, device=DEV: {k: torch.zeros(v.shape, device=device) for k, v in agg.items()}      # noqa: E731


REFUSED = dict(
    **{k: (lambda a, ws, kw={k: v}: _do(a, ws, "fedavg", **kw)) for k, v in dict(clip_threshold=1.0, nonfinite="skip", trim=1, krum=0, rfa=2, defer=True).items()},
    fedopt=lambda a, ws: _do(a, ws, "fedadam", {"current_weights": _like(a)}, {"version": 1}),
    fedbuff=lambda a, ws: _do(a, ws, "fedbuff", do_kw={"version": 1}), feddyn=lambda a, ws: _do(a, ws, "feddyn", alpha=0.01),
    scaffold=lambda a, ws: _do(a, ws, "scaffold", {"weight_dict": {f"e{i:02d}": 1.0 for i in range(5)}, "c_glob": _like(a)},
                               {"control_cache": _cache([_like(a) for _ in ws])}, k=3),
    hierarchy=lambda a, ws: fedbuff.hierarchy_round([(a, ws[0], 5, 0)], version=1), sync_hierarchy=lambda a, ws: sync_hierarchy.sync_hierarchy_round([(_like(a), _cache(ws), 15)], a),
    slab=lambda a, ws: slab.UpdateSlab(a, 2, DEV).put(ws[0]),
    device_cache=lambda a, ws: ingest.DeviceUpdateCache(DEV, placement="slab", capacity=2).__setitem__("e00", S.TR(ws[0], 3)),
    shard_local=lambda a, ws: shard.ShardPlan(_like(a, "meta"), 2, 0, align=8).local(ws[0]),
    shard_slice=lambda a, ws: shard.ShardPlan(_like(a, "meta"), 2, 0, align=8).slice_update(ws[0]),
    key_groups=lambda a, ws: _acc(a, ws, key_groups=[["w"], ["b"]]), scales=lambda a, ws: _acc(a, ws, scales=[1.0, 0.5, 1.0, 1.0, 1.0]),
    dense_mixture=lambda a, ws: _acc(a, ws, lowrank.densify), dtype_mixture=lambda a, ws: _acc(a, ws, lambda w: _with(w, left=w["w"].bfloat16())),
    rank_mismatch=lambda a, ws: _acc(a, ws, lambda w: _with(w, right=w.right["w"][:-1])), shape=lambda a, ws: _acc(a, ws, lambda w: _with(w, left=w["w"][:-1])),
    bf16_aggregate=lambda a, ws: _acc({k: v.bfloat16() for k, v in a.items()}, ws))


@pytest.mark.parametrize("who", list(REFUSED))
def test_refused_before_anything_is_written(who):
    """Every refused caller and every per-key mixture: a TypeError that names low-rank updates, nothing launched, the model's bits untouched."""
    agg = {"w": torch.ones(40, 50, device=DEV), "b": torch.ones(7, device=DEV)}
    ws = [lowrank.compress({"w": torch.full((40, 50), float(i + 1)), "b": torch.ones(7)}, rank=2).to(DEV) for i in range(5)]
    with Launches() as ln:
        with pytest.raises(TypeError, match="(?i)low-rank update.*supported"):
            REFUSED[who](agg, ws)
    assert not ln.names and all(bool((v == 1).all()) for v in agg.values()), ln.names


# ---------------------------------------------------------------------------- residency: engine._staged, engine._Target
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
_CASES = {}


def _lr_case(dtype, shapes="bfg"):      # built once per (dtype, keys), never written
    if (dtype, shapes) not in _CASES:
        _CASES[dtype, shapes] = UC.lowrank_case(dtype, shapes={k: UC.LR_SHAPES[k] for k in shapes})
    return _CASES[dtype, shapes]


@DTYPES
@pytest.mark.parametrize("agg_where", ["gpu", "pageable"])
@pytest.mark.parametrize("where", ["gpu", "pinned", "pageable"])
def test_residency(where, agg_where, dtype):
    """Factors on ``where``, the fp32 aggregate on ``agg_where``; ranks (0, 1, 3, 8, 16) rotated per key.  Client 2's left factor
    of f is a non-contiguous view (an [r, m] tensor transposed): engine._staged copies it, and the caller's tensor stays as it is."""
    base, ups = _lr_case(dtype)
    rates = UC.rates_of(5)
    ws = [UC.lowrank_weights(up, UC.LR_SHAPES, lambda t: UC.place(t, where)) for up in ups]
    ws[2]["f"] = UC.place(ups[2]["f"][0].t().contiguous(), where).t()
    assert ws[2]["f"].shape == (129, 8) and not ws[2]["f"].is_contiguous()
    agg = {k: UC.place(v, agg_where) for k, v in base.items()}
    read, held, objs = UC.snapshot([t for w in ws for t in (*w.values(), *w.right.values())]), UC.snapshot(agg.values()), dict(agg)
    with Launches() as ln:
        engine.accumulate(agg, list(zip(ws, rates)))
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_lowrank"], ln.names
    UC.lowrank_check(f"{where} into {agg_where}", agg, base, ups, rates)
    UC.assert_unchanged("factors", read)
    UC.assert_unchanged("aggregate", held, bytes_too=False)
    assert all(agg[k] is objs[k] and agg[k].is_cuda == (agg_where == "gpu") for k in objs)


# ---------------------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def delay():
    d = SC.Delay()
    yield d
    d.free()


def _late_round(late, call, label, sync, agg, rounds, base, rates):
    """``call(agg, ws)`` once per round of ``rounds`` (lists of LowRankWeights whose factors are revealed late, group = round) under
    the late stream; every round is checked against tests/lowrank_ref.py from the aggregate the round before left."""
    res, before = {}, base
    with late.stream():
        for g, (ups, ws) in enumerate(rounds):
            late.start(g)
            with late.call(f"{label}, round {g}", sync=sync):
                out = call(agg, ws)
            res[f"round{g}"] = late.snap(out)
            late.reuse(*[d for w in ws for d in (w, w.right)])
    late.finish()
    for g, (ups, _) in enumerate(rounds):
        UC.lowrank_check(f"{label} late={not late.ready} round {g}", res[f"round{g}"], before, ups, rates)
        before = {k: v.cpu().numpy() for k, v in res[f"round{g}"].items()}
    return {k: SC.cpu(v) for k, v in res.items()}


@DTYPES
@pytest.mark.parametrize("agg_where", ["gpu", "host"])
def test_late_inputs_on_a_stream_of_their_own(delay, agg_where, dtype):
    """Every factor (and a device aggregate) holds poison until a delay on the test's stream has run.  Into a device aggregate the
    call is asynchronous: the delay must still be running when it returns.  Then the factors are dropped, their blocks
    re-poisoned on the stream, and a second round (the clients in reverse) goes into the same aggregate."""
    base, ups = _lr_case(dtype, "bf")
    shapes, rates = {k: UC.LR_SHAPES[k] for k in "bf"}, UC.rates_of(5)
    sync = None if agg_where == "gpu" else "the host aggregate's write-back (engine._Target.writeback)"

    def case(late):
        agg = {k: late.tensor(torch.from_numpy(v), agg_where) for k, v in base.items()}
        rounds = [(r, [UC.lowrank_weights(up, shapes, lambda t: late.tensor(t, "gpu", g)) for up in r]) for g, r in enumerate((ups, ups[::-1]))]
        return _late_round(late, lambda a, ws: engine.accumulate(a, list(zip(ws, rates))) or a, "low-rank accumulate", sync, agg, rounds, base, rates)
    ready = case(SC.Late(delay, ready=True))
    SC.assert_same("lowrank", ready, case(SC.Late(delay)))


@DTYPES
def test_fedavg_round_on_a_late_stream(delay, dtype):
    base, ups = _lr_case(dtype, "bf")
    shapes = {k: UC.LR_SHAPES[k] for k in "bf"}

    def case(late):
        agg = {k: late.tensor(torch.from_numpy(v)) for k, v in base.items()}
        ws = [UC.lowrank_weights(up, shapes, late.tensor) for up in ups]
        return _late_round(late, lambda a, ws: optimizer_provider.get("fedavg").do(a, _cache(ws, [1, 2, 3, 4, 5]), total=15), "low-rank fedavg", None,
                           agg, [(ups, ws)], base, UC.rates_of(5))
    ready = case(SC.Late(delay, ready=True))
    SC.assert_same("lowrank fedavg", ready, case(SC.Late(delay)))


# ---------------------------------------------------------------------------- client groups and routes
def test_ragged_key_sets_and_two_factor_dtypes():
    """Updates 0, 2 and 3 hold w (fp32 factors), all five hold u (bf16) and x (fp32): one launch for the group (0, 2, 3), one per
    factor dtype for the group of all; every key against the reference over the clients that hold it, at their rates."""
    shapes, carriers = {"w": (129, 127), "u": (31, 33), "x": (32, 32)}, {"w": (0, 2, 3)}
    base, ups = UC.lowrank_case({"w": torch.float32, "u": torch.bfloat16, "x": torch.float32}, shapes=shapes, carriers=carriers)
    agg, rates = {k: torch.from_numpy(v).to(DEV) for k, v in base.items()}, UC.rates_of(5)
    with Launches() as ln:
        engine.accumulate(agg, [(UC.lowrank_weights(up, shapes).to(DEV), r) for up, r in zip(ups, rates)])
    assert ln.names == ["flame_agg_reduce_lowrank"] * 3, ln.names
    UC.lowrank_check("ragged", agg, base, ups, rates)


def test_one_call_three_routes():
    """One accumulate over three client groups: updates 0-2 are SparseWeights (s sparse, c dense), updates 3-5 LowRankWeights (l
    factored, d dense), and all six hold b dense.  s: bitwise tests/sparse_ref.py; l: within the low-rank bound; b, c, d: the bits
    of the round over the dense keys alone.  Then a key that is sparse in one update and factored in another: refused, nothing
    launched, nothing written."""
    from flame_amd import sparse
    g = torch.Generator().manual_seed(5)
    model = {"s": torch.randn(4099, generator=g), "l": torch.randn(129, 127, generator=g), "b": torch.randn(77, generator=g),
             "c": torch.randn(33, generator=g), "d": torch.randn(35, generator=g)}
    raw = [{k: torch.randn(v.shape, generator=g) * 0.01 for k, v in model.items()} for _ in range(6)]
    rates, ups = UC.GROUP_RATES, []
    for c, u in enumerate(raw):
        if c < 3:
            sp = sparse.topk({"s": u["s"]}, ratio=0.05)
            ups.append(sparse.SparseWeights({"s": sp["s"], "b": u["b"], "c": u["c"]}, sp.indices, sp.shapes))
        else:
            lr = lowrank.compress({"l": u["l"]}, rank=(1, 3, 8)[c - 3])
            ups.append(lowrank.LowRankWeights({"l": lr["l"], "b": u["b"], "d": u["d"]}, lr.right, lr.shapes))
    agg = {k: v.to(DEV) for k, v in model.items()}
    with Launches() as ln:
        engine.accumulate(agg, [(u.to(DEV), r) for u, r in zip(ups, rates)])
    assert ln.names == ["flame_sparse_index", "flame_agg_reduce_sparse", "flame_agg_reduce", "flame_agg_reduce_lowrank", "flame_agg_reduce", "flame_agg_reduce"], ln.names
    S.same_bits("s", agg, UC.sparse_want({"s": model["s"].numpy()}, UC.as_numpy(ups[:3], "s") + [{}] * 3, rates))
    UC.lowrank_check("l", agg, {"l": model["l"].numpy()}, [{}] * 3 + [{"l": (u["l"], u.right["l"])} for u in ups[3:]], rates)
    dense = {k: model[k].to(DEV) for k in "bcd"}
    engine.accumulate(dense, [({k: u[k].to(DEV) for k in "bcd" if k in u}, r) for u, r in zip(ups, rates)])
    S.same_bits("dense keys", agg, {k: v.cpu() for k, v in dense.items()})
    # the stated pair of rounds: w sparse + b dense, w factored + b dense; b is bitwise the dense round's in both
    wide = {"w": model["l"], "b": model["b"]}
    as_sparse = lambda u: (lambda sp: sparse.SparseWeights({"w": sp["w"], "b": u["b"]}, sp.indices, sp.shapes))(sparse.topk({"w": u["l"]}, ratio=0.05))      # noqa: E731
    as_lowrank = lambda u: (lambda lr: lowrank.LowRankWeights({"w": lr["l"], "b": u["b"]}, {"w": lr.right["l"]}, {"w": lr.shapes["l"]}))(lowrank.compress({"l": u["l"]}, rank=3))      # noqa: E731
    for make, names in ((as_sparse, ["flame_sparse_index", "flame_agg_reduce_sparse", "flame_agg_reduce"]), (as_lowrank, ["flame_agg_reduce_lowrank", "flame_agg_reduce"])):
        a = {k: v.to(DEV) for k, v in wide.items()}
        with Launches() as ln:
            engine.accumulate(a, [(make(u).to(DEV), r) for u, r in zip(raw, rates)])
        assert ln.names == names, ln.names
        b = {"b": model["b"].to(DEV)}
        engine.accumulate(b, [({"b": u["b"].to(DEV)}, r) for u, r in zip(raw, rates)])
        S.same_bits("b", a, {"b": b["b"].cpu()})
        assert not torch.equal(a["w"].cpu(), wide["w"])
    a = {k: v.to(DEV) for k, v in wide.items()}
    for entries, what in (([as_sparse(raw[0]), as_lowrank(raw[1])], "sparse in update 0 and dense in update 1"),
                          ([as_lowrank(raw[0]), as_sparse(raw[1]), as_sparse(raw[2])], "sparse in update 1 and dense in update 0")):
        with Launches() as ln:
            with pytest.raises(TypeError, match=f"key 'w' is {what}: per-key mixtures of sparse and dense updates are not supported"):
                engine.accumulate(a, [(u.to(DEV), 0.25) for u in entries])
        assert not ln.names
    S.same_bits("refused", a, wide)


# ---------------------------------------------------------------------------- the C entry point, where the engine never goes
@DTYPES
@pytest.mark.parametrize("shape", [(129, 127), (1, 1)], ids=["129x127", "1x1"])
@pytest.mark.parametrize("ranks", [(0, 0, 0), (3, 0, 8)], ids=["rank0", "ranks308"])
def test_out_of_place(ranks, shape, dtype):
    """out != in (the engine always passes in == out), out full of poison with one guard row behind it.  rank0: no k row at all, and
    the tile must still be copied, bit for bit.  ranks308: the reference within the bound.  in keeps its bits, the guard its poison."""
    from flame_amd import _native as N
    (m, n), rates = shape, [0.5, 0.3, 0.2]
    base, ups = UC.lowrank_case(dtype, shapes={"k": shape}, n=3, seed=m, ranks={"k": ranks})
    inp, out = torch.from_numpy(base["k"]).to(DEV), torch.full((m + 1, n), float(SC.POISON), device=DEV)
    left, right = [up["k"][0].to(DEV) for up in ups], [up["k"][1].to(DEV) for up in ups]
    assert all(u.is_contiguous() and v.is_contiguous() and u.shape == (m, r) and v.shape == (r, n) for u, v, r in zip(left, right, ranks))
    meta, n_tiles, n_rows, o = engine.plan_lowrank([(out.data_ptr(), inp.data_ptr(), m, n)], [[t.data_ptr() for t in left]], [[t.data_ptr() for t in right]],
                                                   [list(ranks)], rates, left[0].element_size())
    assert (n_rows == 0) == (not any(ranks)) and n_tiles == -(-m // 128) * -(-n // 128)
    block = torch.from_numpy(meta).to(DEV)
    N.check(N.lib().flame_agg_reduce_lowrank(N.FLAME_F32, engine.dtype_code(dtype), 0, block.data_ptr() + o["segs"], 1, n_tiles, block.data_ptr() + o["rows"],
                                             n_rows, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if any(ranks):
        UC.lowrank_check("out", {"k": out[:m]}, base, ups, rates)
    else:
        S.same_bits("out", {"k": out[:m]}, {"k": torch.from_numpy(base["k"])})
    S.same_bits("in", {"k": inp}, {"k": torch.from_numpy(base["k"])})
    assert bool((out[m] == SC.POISON).all()), "written past m rows"
