"""GPU: server-side Gaussian noise -- flame_noise_fill and the optimizers' ``noise_factor`` / ``noise_seed``.

* Fill: bitwise against tests/noise_ref.py (Philox4x32-10 + Box-Muller restated op for op in numpy
  float32) for 4 dtypes, sizes around the chunk and the block, aligned tensors and views one element
  off alignment, starts 0..5 and 2^34 - 6 (the block index crosses 2^32 inside the key), several keys
  of mixed dtype in one call, four stds (among them fp32-subnormal products and fp16 overflow), a
  sub-range against the slice of the whole, two equal calls; the elements around a view stay untouched.
* Rounds: FedAvg / FedProx / FedAdam over three rounds, tensors and slab slots, with and without
  ``clip_threshold``, ``nonfinite="skip"`` dropping one update: the model is bitwise the C oracle's over
  the (scaled) updates plus the restated noise as a last entry with rate 1.
* Stream contract: a noised FedAvg and a noised FedAdam round under a non-default stream with
  late-written inputs (tests/stream_case.py) give the default-stream bits.
"""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import noise_ref as R
import scenarios as S
import stream_case as SC

pytestmark = [pytest.mark.gpu]
oracle = pytest.mark.oracle

DEV = "cuda:0"
SEED = 1234 | 5678 << 32
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["f32", "bf16", "f16", "f64"]
NUMELS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4099]
STARTS = [0, 1, 2, 3, 4, 5]
FAR = (1 << 34) - 6
STDS = [1.0, 1e-3, 2.0 ** -140, 1e30]
SENTINEL = -7.0


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()
    torch.empty(1, device=DEV)


def _bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def _same(label, got, want):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, label
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{label}: {bad.size} of {g.size} elements differ, first at {bad[:5]}"


def _views(dt, numels, misaligned):
    """Per numel a buffer of sentinels with one spare element at each end and the view to fill: at the
    start of a fresh allocation + one element (misaligned) or + 16 bytes (aligned)."""
    lead = 1 if misaligned else 16 // torch.empty((), dtype=dt).element_size()
    bufs = [torch.full((lead + n + 1,), SENTINEL, dtype=dt, device=DEV) for n in numels]
    views = [b[lead:lead + n] for b, n in zip(bufs, numels)]
    for v, n in zip(views, numels):
        assert n == 0 or (v.data_ptr() % 16 != 0) == misaligned
    return bufs, views, lead


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_fill_bitwise(dt, misaligned):
    """Every (numel, start) pair as one segment of ONE launch per std (56 segments: every size at every
    start 0..5, and two across the 2^32nd block), each segment its own stream."""
    from flame_amd import engine
    cases = [(n, st) for n in NUMELS for st in STARTS] + [(4099, FAR), (4099, FAR - 2)]     # element by element, and vectors
    numels, starts = [c[0] for c in cases], [c[1] for c in cases]
    streams = [3 * i + 1 for i in range(len(cases))]
    for rnd, std in enumerate(STDS):
        bufs, views, lead = _views(dt, numels, misaligned)
        engine.noise_fill_(views, streams, starts, SEED, rnd, std)
        torch.cuda.synchronize()
        for (n, st), sm, b, v in zip(cases, streams, bufs, views):
            label = f"{IDS[DTYPES.index(dt)]}/n{n}/start{st}/std{std:g}"
            _same(label, v, R.fill_torch(v, SEED, rnd, sm, st, std))
            assert bool((b[:lead] == SENTINEL).all()) and bool((b[lead + n:] == SENTINEL).all()), label + ": wrote outside"
    if dt != torch.float64 and not misaligned:
        z = R.fill("f32", SEED, 2, 1, 0, 4099, 2.0 ** -140)
        assert (z != 0).any() and (np.abs(z) < 2.0 ** -126).all()      # the subnormal case is one


def test_fill_mixed_keys_subrange_and_repeat():
    """engine.noise_fill over a model of mixed dtypes: the stream is the key's position counting every
    key, integer and bool keys get nothing; a sub-range filled alone is the slice of the whole; two equal
    calls give equal bits; another round, seed or stream gives other values."""
    from flame_amd import engine
    like = OrderedDict([("a", torch.zeros(4099, device=DEV)), ("n", torch.tensor(3, device=DEV)),
                        ("h", torch.zeros(3, 70, dtype=torch.bfloat16, device=DEV)), ("mask", torch.zeros(5, dtype=torch.bool, device=DEV)),
                        ("d", torch.zeros(1025, dtype=torch.float64, device=DEV)), ("e", torch.zeros(0, device=DEV)),
                        ("s", torch.zeros((), dtype=torch.float16, device=DEV)), ("b", torch.zeros(2051, device=DEV))])
    std = 0.37
    got = engine.noise_fill(like, SEED, 4, std)
    again = engine.noise_fill(like, SEED, 4, std)
    torch.cuda.synchronize()
    assert list(got) == ["a", "h", "d", "e", "s", "b"]
    for pos, (k, t) in enumerate(like.items()):
        if k in got:
            assert got[k].dtype == t.dtype and got[k].shape == t.shape and got[k].device == t.device
            _same(f"mixed/{k}", got[k], R.fill_torch(t.cpu(), SEED, 4, pos, 0, std))
            _same(f"repeat/{k}", again[k], got[k])
    other = [engine.noise_fill(like, SEED, 5, std), engine.noise_fill(like, SEED + 1, 4, std)]
    for o in other:
        assert not bool((o["a"] == got["a"]).any())
    assert not bool((got["a"][:2051] == got["b"]).any())                  # streams 0 and 7
    # [a, b) with start = a, aligned and not, in one launch, against the slice of the whole
    whole = got["a"]
    ranges = [(0, 4099), (4, 1028), (1, 2), (5, 1030), (1024, 4099), (1023, 1025), (3000, 3003)]
    outs = [torch.empty(b - a, device=DEV) for a, b in ranges]
    engine.noise_fill_(outs, [0] * len(ranges), [a for a, _ in ranges], SEED, 4, std)
    torch.cuda.synchronize()
    for (a, b), o in zip(ranges, outs):
        _same(f"subrange[{a}:{b}]", o, whole[a:b])


# ---------------------------------------------------------------------------- rounds
def _drop_in(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _model(g, dt, scale, nbt):
    return OrderedDict([("w", (torch.randn(4099, generator=g, dtype=torch.float64) * scale).to(dt)),
                        ("b", (torch.randn(1025, generator=g, dtype=torch.float64) * scale).to(dt)),
                        ("nbt", torch.tensor(nbt)), ("one", (torch.randn(1, generator=g, dtype=torch.float64) * scale).to(dt))])


def _fill(ups, counts):
    cache = S.SortedCache()
    for i, (u, c) in enumerate(zip(ups, counts)):
        cache[f"e{i:02d}"] = S.TR(u, c)
    return cache


def _on_device(ups, layout):
    if layout == "tensors":
        return [S.to_dev(u, DEV) for u in ups]
    from flame_amd.slab import UpdateSlab
    slab = UpdateSlab(ups[0], len(ups), DEV)
    return [slab.put(S.to_dev(u, DEV)) for u in ups]


ROUND_CASES = [(sort, dt) for sort in ("fedavg", "fedprox", "fedadam") for dt in DTYPES[:3]] + [("fedavg", torch.float64)]


@oracle
@pytest.mark.parametrize("clip", [None, 30.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("layout", ["tensors", "slab"])
@pytest.mark.parametrize("sort,dt", ROUND_CASES, ids=[f"{s}-{IDS[DTYPES.index(d)]}" for s, d in ROUND_CASES])
def test_noised_rounds(sort, dt, layout, clip):
    """Three rounds of 9 updates (round 1 loses one to ``nonfinite="skip"``).  Per round: noise_std is
    s * sqrt(fsum(rate^2)) of the kept rates; the model is bitwise the C oracle's over the kept updates
    (pre-scaled by the recorded clip scales) plus tests/noise_ref.py's noise as a last entry whose count
    is the kept total (rate 1); FedAdam's adaptive rounds from identical state under the FedOPT contract
    (fp32) or bitwise (bf16 / fp16); the int key is the un-noised round's; a second optimizer with the
    same seed reproduces every round bit for bit."""
    from oracle import oracle as O
    s = 0.05
    g = torch.Generator().manual_seed(40 + DTYPES.index(dt))
    kw = {"mu": 0.1} if sort == "fedprox" else {}
    adam = sort == "fedadam"
    guard = {"nonfinite": "skip", **({} if clip is None else {"clip_threshold": clip})}
    opt = _drop_in(sort, noise_factor=s, noise_seed=SEED, **guard, **kw)
    twin = _drop_in(sort, noise_factor=s, noise_seed=SEED, **guard, **kw)
    plain = _drop_in(sort, **guard, **kw)
    ora = O.OracleFedOPT(sort, sqrt_rn=True) if adam else O.OracleFedAvg()
    base = _model(g, dt, 1.0, 3)
    fkeys = [k for k in base if base[k].is_floating_point()]
    dev_base, dev_twin, dev_plain, ora_base = S.to_dev(base, DEV), S.to_dev(base, DEV), S.to_dev(base, DEV), S.to_cpu(base)
    noises = []
    for rnd in range(3):
        n = 9
        ups = [_model(g, dt, 0.1 + 0.1 * i, 10 * rnd + i) for i in range(n)]       # norms from ~7 to ~64: some clipped
        if rnd == 1:
            ups[4]["w"][17] = float("nan")
        counts = [5 + i for i in range(n)]
        total = sum(counts)
        # the float keys of THIS round's base: FedOPT's promotion turns the int64 counter fp32 after the
        # first adaptive round, and a float key of base_weights is noised whatever it was before
        like = OrderedDict((k, torch.empty(v.shape, dtype=v.dtype)) for k, v in dev_base.items())
        int_key = not like["nbt"].is_floating_point()
        got = opt.do(dev_base, _fill(_on_device(ups, layout), counts), total=total)
        got2 = twin.do(dev_twin, _fill(_on_device(ups, layout), counts), total=total)
        unnoised = plain.do(dev_plain, _fill(_on_device(ups, layout), counts), total=total)
        recs = opt.update_stats
        kept = [i for i, r in enumerate(recs) if not r.skipped]
        assert kept == ([i for i in range(n) if i != 4] if rnd == 1 else list(range(n)))
        if clip is not None:
            assert any(recs[i].scale < 1.0 for i in kept) and any(recs[i].scale == 1.0 for i in kept)
        kept_total = sum(counts[i] for i in kept)
        rates = [counts[i] / kept_total for i in kept]
        std = s * math.sqrt(math.fsum(r * r for r in rates))
        assert opt.noise_std == std and opt.noise_round == rnd + 1 and twin.noise_round == rnd + 1
        noise = OrderedDict((k, R.fill_torch(v, SEED, rnd, pos, 0, std)) for pos, (k, v) in enumerate(like.items())
                            if v.is_floating_point())
        noises.append(noise)
        scaled = [OrderedDict((k, O.tmp_tensor(v, recs[i].scale) if v.is_floating_point() else v.clone())
                              for k, v in ups[i].items()) for i in kept]
        cache = _fill(scaled, [counts[i] for i in kept])
        cache["zz_noise"] = S.TR(noise, kept_total)                 # sorts last; rate kept_total / kept_total = 1
        exp = ora.do(ora_base, cache, total=kept_total)
        label = f"{sort}/{layout}/r{rnd}"
        S.assert_bitwise(label + "/avg", {k: dev_base[k] for k in base}, {k: ora_base[k] for k in base})
        if adam and dt == torch.float32 and rnd > 0:
            S.assert_close_fedopt(label, {k: got[k] for k in fkeys}, {k: exp[k] for k in fkeys})
        elif adam and rnd > 0:
            S.assert_bitwise(label + "/cur", {k: got[k] for k in fkeys}, {k: exp[k] for k in fkeys})
        else:
            S.assert_bitwise(label + "/cur", {k: got[k] for k in base}, {k: exp[k] for k in base})
        S.assert_bitwise(label + "/twin", {k: got2[k] for k in got}, S.to_cpu({k: got[k] for k in got}))
        S.assert_bitwise(label + "/twin avg", {k: dev_twin[k] for k in base}, S.to_cpu({k: dev_base[k] for k in base}))
        if int_key:
            assert torch.equal(dev_base["nbt"].cpu(), dev_plain["nbt"].cpu()) and torch.equal(got["nbt"].cpu(), unnoised["nbt"].cpu())
        assert not torch.equal(dev_base["w"].cpu(), dev_plain["w"].cpu())         # the noise did land
        if adam:
            # the next round starts from a copy of the new current, as the roles do; the oracle and
            # the un-noised optimizer take the drop-in's state: every round from identical state
            dev_base, dev_twin = {k: v.clone() for k, v in got.items()}, {k: v.clone() for k, v in got2.items()}
            dev_plain = {k: v.clone() for k, v in unnoised.items()}
            ora_base = S.to_cpu(got)
            ora.current_weights = S.to_cpu(got)
            if opt.m_t is not None:
                ora.m_t, ora.v_t = S.to_cpu(opt.m_t), S.to_cpu(opt.v_t)
    # rounds draw different noise (a 16-bit value may coincide here and there: count, do not forbid)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert int((noises[a]["w"] == noises[b]["w"]).sum()) < 4099 // 8


# ---------------------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def delay():
    d = SC.Delay()
    yield d
    d.free()


def _stream_data():
    g = torch.Generator().manual_seed(77)
    base = _model(g, torch.float32, 1.0, 3)
    base["h"] = torch.randn(2053, generator=g).to(torch.bfloat16)
    ups = []
    for i in range(7):
        u = _model(g, torch.float32, 0.01, 100 + i)
        u["h"] = (torch.randn(2053, generator=g) * 0.01).to(torch.bfloat16)
        ups.append(u)
    return base, ups, [3, 1, 4, 1, 5, 9, 2]


@oracle
@pytest.mark.parametrize("sort", ["fedavg", "fedadam"])
def test_noised_round_on_a_late_stream(sort, delay):
    """One noised round with every input poisoned until late on a stream of its own: asynchronous (the
    delay is still running when ``do()`` returns), the FedAvg result bitwise the oracle's with the
    restated noise, and everything bitwise the default-stream run.  FedAdam: the fused round (state
    set by hand, as the roles hand over a copy of the last current), noise as the launch's last client."""
    from oracle import oracle as O
    base0, ups, counts = _stream_data()
    total, s = sum(counts), 0.02
    std = s * math.sqrt(math.fsum((c / total) ** 2 for c in counts))
    noise = OrderedDict((k, R.fill_torch(v, SEED, 0, list(base0).index(k), 0, std)) for k, v in base0.items()
                        if v.is_floating_point())
    cache = _fill([OrderedDict((k, v.clone()) for k, v in u.items()) for u in ups], counts)
    cache["zz_noise"] = S.TR(noise, total)
    exp_avg = O.OracleFedAvg().do(OrderedDict((k, v.clone()) for k, v in base0.items()), cache, total=total)

    def case(L):
        opt = _drop_in(sort, noise_factor=s, noise_seed=SEED)
        base, srcs = L.weights(base0), [L.weights(u) for u in ups]
        cur = L.weights(base0) if sort == "fedadam" else None
        with L.stream():
            if cur is not None:
                opt.current_weights = cur
            L.start()
            with L.call(f"noise/{sort}"):
                out = opt.do(base, _fill([OrderedDict(u) for u in srcs], counts), total=total)
            L.reuse(*srcs)
            res = {"avg": L.snap(base), "out": L.snap(out)}
            if sort == "fedadam":
                res["m"], res["v"] = L.snap(opt.m_t), L.snap(opt.v_t)
        L.finish()
        assert opt.noise_round == 1 and opt.noise_std == std
        S.assert_bitwise(f"noise/{sort}/avg", res["avg"], exp_avg)
        return res
    ready = case(SC.Late(delay, ready=True))
    late = case(SC.Late(delay))
    SC.assert_same(f"noise/{sort}", ready, late)
