"""flame_agg_reduce_lowrank on the GPU against tests/lowrank_ref.py ("the low-rank contract"): the shapes,
ranks, alignments and values at which the tiled product can go wrong; the densified equivalence; the refusals."""
import numpy as np
import pytest
import torch

import lowrank_ref
import scenarios as S
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
