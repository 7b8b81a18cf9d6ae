"""flame_agg_reduce_sign on the GPU, BITWISE against tests/sign_ref.py ("the sign contract"): the sizes at which a tile,
a word or a block ends, client counts either side of the unroll, every scale the rule speaks of, pad bits set, sentinels round every key."""
import numpy as np
import pytest
import torch

import scenarios as S
import sign_ref
import stream_case as SC
import test_gpu_lowrank as LR
from flame_amd import _native as N, engine, sign
from flame_amd.optimizers import optimizer_provider
from large_case import Launches
from test_mx_host import _cache

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
NUMELS = {f"k{m}": m for m in (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16384 + 37)}
SPECIAL = np.array([0.0, 1e-41, 2.0 ** -126, 1.0, 3e38, np.inf, -0.75, np.nan], dtype=np.float32)
GUARD, _CASES = 5, {}
PLACES = {"gpu": lambda t: t.to(DEV), "pinned": lambda t: t.clone().pin_memory(), "pageable": lambda t: t.clone()}


def _case(n, keys=tuple(NUMELS)):        # (base, ups[c][k] = (bits, scales), rates, want), built once and never written
    if (n, keys) not in _CASES:
        rng = np.random.default_rng(n)
        base, ups = {}, [{} for _ in range(n)]
        for k in keys:
            m = NUMELS[k]
            base[k] = (rng.choice([-1.0, 1.0], m) * 2.0 ** rng.uniform(-20, 20, m)).astype(np.float32)
            base[k][::5], base[k][3::97] = -0.0, 3e38
            for c, up in enumerate(ups):
                bits = rng.integers(0, 256, 8 * -(-m // 64), dtype=np.uint8)
                pad = np.packbits(np.arange(bits.size * 8) >= m, bitorder="little")       # every pad bit of the last word is set
                scales = (2.0 ** rng.uniform(-20, 20, -(-m // 256))).astype(np.float32)
                if scales.size >= 16:       # each special in a block of its own, one of three by client: a NaN in three blocks only
                    scales[(3 * np.arange(8) + c % 3) % scales.size] = SPECIAL
                up[k] = (bits | pad, scales)
        rates = [(1.0, 0.75, 0.5)[c % 3] for c in range(n)]
        want = {k: torch.from_numpy(sign_ref.accumulate(base[k], [u[k] for u in ups], rates)) for k in base}
        _CASES[n, keys] = (base, ups, rates, want)
    return _CASES[n, keys]


_off4 = lambda t: torch.cat([torch.zeros(4, dtype=torch.uint8), t]).to(DEV)[4:]       # noqa: E731  (a view 4 bytes into its buffer)


def _weights(up, place, bits=None):
    return sign.SignWeights({k: (bits or place)(torch.from_numpy(b)) for k, (b, _) in up.items()},
                            {k: place(torch.from_numpy(s)) for k, (_, s) in up.items()}, {k: (NUMELS[k],) for k in up})


def _guarded(base):     # {k: a view of the key inside a buffer of sentinels}, and the check of both once the round has run
    bufs = {k: torch.full((v.size + 2 * GUARD,), float(SC.POISON), device=DEV) for k, v in base.items()}
    agg = {k: b[GUARD:GUARD + base[k].size].copy_(torch.from_numpy(base[k])) for k, b in bufs.items()}

    def check(label, want):
        S.same_bits(label, agg, want)
        assert all(bool((torch.cat([b[:GUARD], b[GUARD + agg[k].numel():]]) == SC.POISON).all()) for k, b in bufs.items()), f"{label}: written outside a key"
    return agg, check


@pytest.mark.parametrize("n,where", [(n, "gpu") for n in (1, 2, 8, 9, 65)] + [(9, w) for w in ("pinned", "pageable", "misaligned")])
def test_reduce_matches_the_contract(n, where):
    """One launch over the eleven keys; sums overflow to inf, a NaN where the reference has one.  misaligned: the engine copies the bits."""
    base, ups, rates, want = _case(n)
    ws = [_weights(u, PLACES.get(where, PLACES["gpu"]), _off4 if where == "misaligned" else None) for u in ups]
    assert where != "misaligned" or all(w[k].data_ptr() % 8 == 4 for w in ws for k in NUMELS)
    assert all(bool(f(want["k4097"]).any()) for f in (torch.isinf, torch.isnan, torch.isfinite)) and not bool(torch.isnan(want["k257"]).any())
    agg, check = _guarded(base)
    with Launches() as ln:
        engine.accumulate(agg, list(zip(ws, rates)))
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_sign"], ln.names
    check(f"sign n={n} {where}", want)


def test_key_set_groups():
    """k4097 is in all four updates, k257 in updates 1 and 3 only: two launches, each over its own clients and rates."""
    base, ups, _, _ = _case(4, ("k257", "k4097"))
    rates = [0.5, 0.25, 0.125, 2.0]
    ups = [{k: v for k, v in u.items() if k == "k4097" or c % 2} for c, u in enumerate(ups)]
    want = {"k4097": sign_ref.accumulate(base["k4097"], [u["k4097"] for u in ups], rates),
            "k257": sign_ref.accumulate(base["k257"], [ups[1]["k257"], ups[3]["k257"]], [0.25, 2.0])}
    agg, check = _guarded(base)
    with Launches() as ln:
        engine.accumulate(agg, [(_weights(u, PLACES["gpu"]), r) for u, r in zip(ups, rates)])
    assert ln.names == ["flame_agg_reduce_sign"] * 2, ln.names
    check("groups", {k: torch.from_numpy(v) for k, v in want.items()})


def test_late_inputs_on_a_stream_of_their_own():
    """Bits, scales and the aggregate hold poison until a delay on the test's stream has run (tests/stream_case.py)."""
    base, ups, rates, want = _case(9, ("k65", "k4097", "k16421"))
    delay = SC.Delay()

    def case(late):
        agg = late.weights({k: torch.from_numpy(v) for k, v in base.items()})
        ws = [_weights(u, lambda t: late.tensor(t.clone())) for u in ups]
        with late.stream():
            late.start()
            with late.call("sign accumulate"):
                engine.accumulate(agg, list(zip(ws, rates)))
            res = late.snap(agg)
        late.finish()
        S.same_bits(f"late={not late.ready}", res, want)
        return {"out": SC.cpu(res)}
    SC.assert_same("sign", case(SC.Late(delay, ready=True)), case(SC.Late(delay)))
    delay.free()


def test_out_of_place_through_the_entry_point():
    """out != in over engine.plan_sign's table: out is the reference between its sentinels, in keeps its bits."""
    base, ups, rates, want = _case(9, ("k1", "k4097", "k16421"))
    ins = {k: torch.from_numpy(v).to(DEV) for k, v in base.items()}
    outs, check = _guarded({k: np.full_like(v, 5.0) for k, v in base.items()})
    ws = [_weights(u, PLACES["gpu"]) for u in ups]
    segs = [engine.Seg(ins[k].numel(), out=outs[k].data_ptr(), inp=ins[k].data_ptr()) for k in base]
    meta, n_chunks, o = engine.plan_sign(segs, [[w[k].data_ptr() for w in ws] for k in base], [[w.scales[k].data_ptr() for w in ws] for k in base], rates)
    block = torch.from_numpy(meta).to(DEV)
    b = block.data_ptr()
    N.check(N.lib().flame_agg_reduce_sign(N.FLAME_F32, 0, b, len(segs), n_chunks, b + o["bits"], b + o["scales"], len(ws), b + o["r32"],
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check("out", want)
    S.same_bits("in", ins, {k: torch.from_numpy(v) for k, v in base.items()})


@pytest.mark.parametrize("sort", ["fedavg", "fedprox", "fedgft"])
def test_optimizer_round_equals_the_round_over_the_dequantized_updates(sort):
    """Two sign keys, a dense key (under min_numel) and an int key in one round: one sign launch beside the dense launches."""
    g = torch.Generator().manual_seed(11)
    model = {"w": torch.randn(3, 4099, generator=g), "v": torch.randn(300, generator=g), "b": torch.randn(77, generator=g), "n": torch.tensor(3)}
    ups = [sign.compress({k: torch.randn(v.shape, generator=g).to(v.dtype) for k, v in model.items()}, min_numel=100) for _ in range(4)]
    kw = {"fedprox": {"mu": 0.1}, "fedgft": {"fair": "SP", "gamma": 0.1}}.get(sort, {})
    out = []
    for dense in (False, True):
        ws = [{k: v.to(DEV) for k, v in sign.dequantize(u).items()} if dense else u.to(DEV) for u in ups]
        with Launches() as ln:
            out.append(optimizer_provider.get(sort, **kw).do({k: v.to(DEV) for k, v in model.items()}, _cache(ws, [2, 3, 4, 5]), total=14))
        assert dense or (ln.count("flame_agg_reduce_sign"), ln.count("flame_agg_reduce")) == (1, 2) and ln.names[0] == "flame_agg_reduce_sign", ln.names
    S.same_bits(f"{sort} sign vs dequantize", out[0], {k: v.cpu() for k, v in out[1].items()})
    assert list(ups[0].scales) == ["w", "v"] and not torch.equal(out[0]["w"].cpu(), model["w"])


REFUSED = {**{k: v for k, v in LR.REFUSED.items() if k not in ("dense_mixture", "dtype_mixture", "rank_mismatch", "shape")},
           "dense_mixture": lambda a, ws: LR._acc(a, ws, sign.dequantize), "f16_aggregate": lambda a, ws: LR._acc({k: v.half() for k, v in a.items()}, ws)}


@pytest.mark.parametrize("who", list(REFUSED))
def test_refused_before_anything_is_written(who):
    """Every refused caller (the low-rank test's table of them) and the mixtures: a TypeError that names sign updates, nothing launched."""
    agg = {"w": torch.ones(40, 50, device=DEV), "b": torch.ones(7, device=DEV)}
    ws = [sign.compress({"w": torch.full((40, 50), float(i + 1)), "b": torch.ones(7)}).to(DEV) for i in range(5)]
    with Launches() as ln:
        with pytest.raises(TypeError, match="(?i)sign update.*supported"):
            REFUSED[who](agg, ws)
    assert not ln.names and all(bool((v == 1).all()) for v in agg.values()), ln.names
