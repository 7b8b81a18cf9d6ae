"""GPU: the geometric median (RFA) -- flame_update_dist, engine.update_dist and the optimizers'
``rfa`` / ``rfa_nu`` kwargs.

* Distances: each ``dist2[i]`` against ``math.fsum`` of the fp64 terms (tests/rfa_ref.py), relative
  error ``<= (elements + 8) * 2^-53``.  Derived, not measured: the terms are non-negative, so a sum
  of ``elements`` of them in any order is within ``(elements - 1) u`` of exact (Higham), each term
  carries up to 3 roundings on each side (the subtract, the square, and the add or the reference's
  conversion) which the two sides may place differently, and the reference rounds once at the end;
  ``u = 2^-53``.  The observed error is printed.
* Zero centre: bitwise ``engine.update_stats``.  Centre = client j: ``dist2[j] == 0.0`` exactly.
* Optimizers: from ``rfa_trace`` every iteration's centre is rebuilt with the oracle's reduction
  from the reported weights, the next reported distances are checked against the fsum reference of
  that centre, the weights against tests/rfa_ref.py of the reported distances (exactly), and the
  model bitwise against the oracle with the final weights as rates.

Every optimizer test consults the CPU oracle, so the branches they reach are credited.
"""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import rfa_ref as R
import scenarios as S

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DEV = "cuda:0"
U53 = 2.0 ** -53
SIZES = [1023, 0, 1, 3, 1024, 4099, 70001]
N_EL = sum(SIZES)
TOL = (N_EL + 8) * U53
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["f32", "bf16", "f16", "f64"]
LAYOUTS = ["tensors", "slab", "misaligned"]
NS = [1, 8, 9, 65]                      # the 8-client group, its remainder loop, the 64-client LDS batch


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()


def _oracle():
    from oracle import oracle as O
    return O


def _drop_in(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _misaligned(v):
    buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=DEV)
    buf[1:].copy_(v.reshape(-1))
    out = buf[1:].view(v.shape)
    assert v.numel() == 0 or out.data_ptr() % 16 != 0
    return out


def _layout(ups, layout):
    """The same updates on the GPU as plain tensors, UpdateSlab slots (tiled), or views one element
    off 16-byte alignment (the bounded element loads)."""
    if layout == "tensors":
        return [S.to_dev(w, DEV) for w in ups], None
    if layout == "misaligned":
        return [{k: _misaligned(v) for k, v in w.items()} for w in ups], None
    from flame_amd.slab import UpdateSlab
    slab = UpdateSlab(ups[0], len(ups), DEV)
    return [slab.put(S.to_dev(w, DEV)) for w in ups], slab


def _centre(z, layout):
    return {k: (_misaligned(v) if layout == "misaligned" else v.to(DEV)) for k, v in z.items()}


def _fill(ups, counts=None):
    cache = S.SortedCache()
    for i, u in enumerate(ups):
        cache[f"e{i:04d}"] = S.TR(u, 1 if counts is None else counts[i])
    return cache


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _within(label, got, ref, tol=TOL):
    worst = 0.0
    for g, r in zip(got, ref):
        if not math.isfinite(r):
            assert (math.isnan(g) and math.isnan(r)) or g == r, (label, g, r)
            continue
        err = abs(g - r) / r if r else abs(g)
        worst = max(worst, err)
    print(f"{label}: max relative error {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol, f"{label}: {worst:.3e} > {tol:.3e}"


def _oracle_sum(out, xs, w):
    """FLAME_AGG_INIT_FIRST as the oracle states it: ``out = tmp_0`` (fedbuff.py:139-140), then the
    other updates are added in order."""
    O = _oracle()
    O.reduce_tensor(out, xs[:1], w[:1], init_first=True)
    if len(xs) > 1:
        O.reduce_tensor(out, xs[1:], w[1:])


def _check_centre(label, ws, ups, w):
    """A Weiszfeld step's other half on these very device updates: the centre ``sum_i w_i x_i``
    (optimizer/rfa.py's ``centre``: the existing reduction, FLAME_AGG_INIT_FIRST) is bitwise the
    oracle's reduce_tensor with the same weights, key by key."""
    from flame_amd.optimizer import rfa
    O = _oracle()
    z = rfa.centre(ws, w)
    fkeys = [k for k in ups[0] if ups[0][k].is_floating_point()]
    assert list(z) == fkeys, label
    exp = {k: torch.empty_like(ups[0][k]) for k in fkeys}
    for k in fkeys:
        _oracle_sum(exp[k], [u[k] for u in ups], list(w))
    S.assert_bitwise(label, z, exp)
    return z


class _Launches:
    """Names of the native launches made inside the block (engine._recorders)."""

    def __enter__(self):
        from flame_amd import engine
        self.events = []
        engine._recorders.append(self.events)
        return self

    def __exit__(self, *exc):
        from flame_amd import engine
        engine._recorders.remove(self.events)
        self.names = [ev[0] for ev in self.events]
        return False

    def count(self, name):
        return sum(1 for n in self.names if n == name)


# ---------------------------------------------------------------------------- 1. the kernel
_BANK = {}


def _bank(dt):
    """65 updates N(0, 1) * (0.5 + 0.01 i) over SIZES in ``dt``, a random centre of the dtype, and
    the fsum reference of every update's distance to it: built once per dtype, never modified."""
    if dt not in _BANK:
        g = torch.Generator().manual_seed(900 + DTYPES.index(dt))
        ups = [{f"k{j}": (torch.randn(s, generator=g) * (0.5 + 0.01 * i)).to(dt) for j, s in enumerate(SIZES)}
               for i in range(max(NS))]
        z = {f"k{j}": (0.3 * torch.randn(s, generator=g)).to(dt) for j, s in enumerate(SIZES)}
        _BANK[dt] = (ups, z, R.dist2(ups, z)[0])
    return _BANK[dt]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_distances_within_the_any_order_bound(dt, layout):
    from flame_amd import engine
    ups, z, ref = _bank(dt)
    for n in NS:
        label = f"{IDS[DTYPES.index(dt)]}/{layout}/n{n}"
        ws, slab = _layout(ups[:n], layout)
        zc = _centre(z, layout)
        d2, nf = engine.update_dist(ws, zc, DEV)
        assert d2.dtype == np.float64 and d2.shape == (n,) and nf.dtype == np.int64 and nf.shape == (n,), label
        assert not nf.any(), label
        _within(label, d2.tolist(), ref[:n])
        again, nf2 = engine.update_dist(ws, zc, DEV)                    # equal launches, equal bits
        assert np.array_equal(_bits(d2), _bits(again)) and np.array_equal(nf, nf2), label
        # a zero centre, +0 and -0 mixed: bitwise the statistics pass
        zero = {k: torch.zeros_like(v) for k, v in z.items()}
        for v in zero.values():
            v.reshape(-1)[::2] = -0.0
        sumsq, nf_s = engine.update_stats(ws, DEV)
        d0, nf0 = engine.update_dist(ws, _centre(zero, layout), DEV)
        assert np.array_equal(_bits(d0), _bits(sumsq)) and np.array_equal(nf0, nf_s), label
        # the centre equal to client j: exactly 0 there
        j = n // 2
        dj, _ = engine.update_dist(ws, _centre(ups[j], layout), DEV)
        assert dj[j] == 0.0 and (n == 1 or (np.delete(dj, j) > 0).all()), label
        # one Weiszfeld step from these distances: the centre is the oracle's
        _check_centre(label, ws, ups[:n], R.weights(d0.tolist(), 1e-6, None))
        del ws, slab


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_special_values(dt):
    """NaN and +-inf in a whole aligned chunk (the vector loads), in the tail chunk (the bounded
    loads) and, under the misaligned layout, in element-wise reads: counts exact, term 0 -- the
    distances are bitwise those of the same updates with the planted elements replaced by the
    centre's value (d = 0 adds nothing).  One inf centre element: +inf for every client finite
    there, nothing counted.  f64 1e308 against a negative centre: +inf, never NaN."""
    from flame_amd import engine
    n = 9
    T = engine.chunk_elems(engine.dtype_code(dt))
    numel = 2 * T + 37
    g = torch.Generator().manual_seed(40 + DTYPES.index(dt))
    xs = [torch.randn(numel, generator=g).to(dt) for _ in range(n)]
    z = (0.5 * torch.randn(numel, generator=g)).to(dt)
    clean = [x.clone() for x in xs]
    want_nf = [0] * n
    for off in (5, T + 200, 2 * T + 3):
        for k, v in enumerate((math.nan, math.inf, -math.inf)):
            for u in range(k + 1):
                i = (off + k + 2 * u) % n
                xs[i][off + 3 * k] = v
                clean[i][off + 3 * k] = z[off + 3 * k]
                want_nf[i] += 1
    assert sum(want_nf) == 18
    ref, ref_nf = R.dist2([{"x": x} for x in xs], {"x": z})
    assert ref_nf == want_nf
    for layout in LAYOUTS:
        ws, slab = _layout([{"x": x} for x in xs], layout)
        cs, cslab = _layout([{"x": x} for x in clean], layout)
        zc = _centre({"x": z}, layout)
        d2, nf = engine.update_dist(ws, zc, DEV)
        dc, nfc = engine.update_dist(cs, zc, DEV)
        assert nf.tolist() == want_nf and not nfc.any(), layout
        assert np.array_equal(_bits(d2), _bits(dc)), layout
        _within(f"special/{layout}", d2.tolist(), ref, (numel + 8) * U53)
        # one inf element of the centre, where client 0 holds a NaN and the others are finite
        zi = z.clone()
        zi[5] = math.inf
        assert math.isnan(float(xs[5 % n][5])) and want_nf[5 % n] > 0
        di, nfi = engine.update_dist(ws, _centre({"x": zi}, layout), DEV)
        holder = 5 % n
        assert nfi.tolist() == want_nf, layout
        assert all(di[i] == math.inf for i in range(n) if i != holder) and di[holder] == d2[holder], (layout, di)
        zn = z.clone()
        zn[T + 1] = math.nan
        dn, _ = engine.update_dist(ws, _centre({"x": zn}, layout), DEV)
        assert np.isnan(dn).all(), layout
        _check_centre(f"special/{layout}", cs, [{"x": x} for x in clean], [1.0 / n] * n)
        del ws, slab, cs, cslab
    if dt == torch.float64:
        big = [{"x": torch.full((T + 5,), 1e308, dtype=dt)}, {"x": torch.full((T + 5,), -1e308, dtype=dt)},
               {"x": torch.zeros(T + 5, dtype=dt)}]
        zc = {"x": torch.full((T + 5,), -1e308, dtype=dt, device=DEV)}
        d2, nf = engine.update_dist([S.to_dev(w, DEV) for w in big], zc, DEV)
        assert d2[0] == math.inf and d2[1] == 0.0 and d2[2] == math.inf and not nf.any()


def test_two_dtype_model_ignored_keys_and_ragged_sets():
    """f32 and bf16 keys (two launches accumulate into one output), an int64 0-dim key and a bool
    mask that take no part; as tensors and as slab slots of a DeviceUpdateCache; ragged key sets are
    measured over the keys each update carries; a centre that lacks a key or holds another dtype or
    shape is refused by name."""
    from flame_amd import engine
    from flame_amd.ingest import DeviceUpdateCache
    g = torch.Generator().manual_seed(5)
    ups = []
    for i in range(9):
        ups.append({"a": torch.randn(4099, generator=g), "nbt": torch.tensor(7 + i),
                    "b": torch.randn(3 * 2048 + 5, generator=g).bfloat16(),
                    "mask": torch.rand(33, generator=g) > 0.5, "c": torch.randn(17, 3, generator=g)})
    z = {"a": torch.randn(4099, generator=g), "b": torch.randn(3 * 2048 + 5, generator=g).bfloat16(),
         "c": torch.randn(17, 3, generator=g), "unused": torch.zeros(3)}
    ref, _ = R.dist2(ups, z)
    tol = (4099 + 3 * 2048 + 5 + 51 + 8) * U53
    zc = S.to_dev(z, DEV)
    with _Launches() as ln:
        d2, nf = engine.update_dist([S.to_dev(w, DEV) for w in ups], zc, DEV)
    assert ln.count("flame_update_dist") == 2 and ln.count("flame_update_stats") == 0, ln.names
    _within("two-dtype", d2.tolist(), ref, tol)
    assert not nf.any()
    cache = DeviceUpdateCache(device=DEV, placement="slab", capacity=9)
    for i, w in enumerate(ups):
        cache[f"e{i}"] = S.TR({k: v.clone() for k, v in w.items()}, 1)
    d3, nf3 = engine.update_dist([cache[f"e{i}"].weights for i in range(9)], zc, DEV)
    _within("two-dtype/slots", d3.tolist(), ref, tol)
    fl = [{k: v for k, v in w.items() if v.is_floating_point()} for w in ups]
    _check_centre("two-dtype", [S.to_dev(w, DEV) for w in ups], fl, R.weights(d2.tolist(), 1e-6, None))
    # a host-resident centre and host-resident updates give the device's bits
    d4, _ = engine.update_dist([{k: v.clone() for k, v in w.items()} for w in ups], z, DEV)
    assert np.array_equal(_bits(d4), _bits(d2))
    # ragged: update 3 lacks "b", update 5 lacks "c"
    rag = [dict(w) for w in ups]
    del rag[3]["b"], rag[5]["c"]
    ref_r, _ = R.dist2(rag, z)
    dr, _ = engine.update_dist([S.to_dev(w, DEV) for w in rag], zc, DEV)
    _within("ragged", dr.tolist(), ref_r, tol)
    assert dr[3] < d2[3] and dr[5] < d2[5] and dr[0] == d2[0]
    for bad, name in (({k: v for k, v in zc.items() if k != "b"}, "'b'"), (dict(zc, a=zc["a"].double()), "'a'"),
                      (dict(zc, c=zc["c"].reshape(3, 17)), "'c'")):
        with pytest.raises(ValueError, match=name):
            engine.update_dist([S.to_dev(w, DEV) for w in ups], bad, DEV)


# ---------------------------------------------------------------------------- 2. optimizers
def _model(gen, n, dt, ints):
    mu = {"k0": torch.randn(4099, generator=gen), "k1": torch.randn(210, generator=gen)}
    ups = []
    for i in range(n):
        scale = -3.0 if i == 4 else 1.0                      # one update far away
        u = {k: (scale * v + 0.1 * torch.randn(v.shape, generator=gen)).to(dt) for k, v in mu.items()}
        if ints:
            u["nbt"] = torch.tensor(100 + 37 * i)
        ups.append(u)
    return ups


def _check_trace(label, opt, ups, elig, fkeys, nu=1e-6):
    """Every iteration of ``opt.rfa_trace`` over the eligible updates ``elig`` (positions in ``ups``)."""
    O = _oracle()
    xs = [ups[i] for i in elig]
    n_el = sum(xs[0][k].numel() for k in fkeys)
    prev = [1.0 / len(xs)] * len(xs)
    z = {k: torch.zeros_like(xs[0][k]) for k in fkeys}
    for t, (d2, w) in enumerate(opt.rfa_trace):
        _within(f"{label}/t{t + 1}", list(d2), R.dist2([{k: x[k] for k in fkeys} for x in xs], z)[0], (n_el + 8) * U53)
        assert list(w) == R.weights(d2, nu, prev), (label, t)
        prev = list(w)
        z = {k: torch.empty_like(xs[0][k]) for k in fkeys}
        for k in fkeys:
            _oracle_sum(z[k], [x[k] for x in xs], list(w))
    return prev


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("sort", ["fedavg", "fedprox", "fedadam"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=IDS[:3])
def test_rfa_optimizers_three_rounds(sort, dt, T):
    O = _oracle()
    n = 9
    g = torch.Generator().manual_seed(61 + DTYPES.index(dt))
    kw = {"mu": 0.1} if sort == "fedprox" else {}
    adam = sort == "fedadam"
    opt = _drop_in(sort, rfa=T, **kw)
    ora = O.OracleFedOPT(sort, sqrt_rn=True) if adam else O.OracleFedAvg()
    base = {"k0": torch.randn(4099, generator=g).to(dt), "k1": torch.randn(210, generator=g).to(dt)}
    if not adam:
        base["nbt"] = torch.tensor(7)
    fkeys = ("k0", "k1")
    dev_base, ora_base = S.to_dev(base, DEV), S.to_cpu(base)
    for rnd in range(3):
        ups = _model(g, n, dt, not adam)
        counts = [5 + i for i in range(n)]                   # counts play no part
        with _Launches() as ln:
            got = opt.do(dev_base, _fill([S.to_dev(u, DEV) for u in ups], counts), total=sum(counts))
        label = f"{sort}/{IDS[DTYPES.index(dt)]}/T{T}/r{rnd}"
        assert ln.count("flame_update_stats") == 1 and ln.count("flame_update_dist") == T - 1, ln.names
        assert len(opt.rfa_trace) == T and opt.update_stats == []
        w = _check_trace(label, opt, ups, list(range(n)), fkeys)
        recs = opt.rfa_records
        assert [r.end for r in recs] == [f"e{i:04d}" for i in range(n)] and [r.weight for r in recs] == w
        assert w[4] == min(w) and abs(math.fsum(w) - 1.0) < 1e-15, label
        # the model: the oracle's round with the final weights as rates (count = w_i, total = 1)
        exp = ora.do(ora_base, _fill([S.to_cpu(u) for u in ups], w), total=1.0)
        S.assert_bitwise(f"{label}/avg", {k: dev_base[k] for k in base}, {k: ora_base[k] for k in base})
        if adam and dt == torch.float32 and rnd > 0:
            S.assert_close_fedopt(label, {k: got[k] for k in fkeys}, {k: exp[k] for k in fkeys})
        elif adam and rnd > 0:
            S.assert_bitwise(f"{label}/cur", {k: got[k] for k in fkeys}, {k: exp[k] for k in fkeys})
        else:
            S.assert_bitwise(f"{label}/cur", {k: got[k] for k in base}, {k: exp[k] for k in base})
        if adam:
            dev_base = {k: v.clone() for k, v in got.items()}
            ora_base = S.to_cpu(got)
            ora.current_weights = S.to_cpu(got)
            if opt.m_t is not None:
                ora.m_t, ora.v_t = S.to_cpu(opt.m_t), S.to_cpu(opt.v_t)


@pytest.mark.parametrize("policy", ["keep", "skip", "raise"])
def test_nonfinite_policies_with_one_poisoned_update(policy):
    O = _oracle()
    n, bad = 9, 6
    g = torch.Generator().manual_seed(88)
    ups = _model(g, n, torch.float32, True)
    ups[bad]["k0"][1234] = math.inf
    base = {"k0": torch.randn(4099, generator=g), "k1": torch.randn(210, generator=g), "nbt": torch.tensor(7)}
    opt = _drop_in("fedavg", rfa=3, nonfinite=policy)
    dev = S.to_dev(base, DEV)
    if policy == "raise":
        with pytest.raises(ValueError, match=f"e{bad:04d}"):
            opt.do(dev, _fill([S.to_dev(u, DEV) for u in ups]), total=n)
        assert [r.nonfinite for r in opt.update_stats] == [int(i == bad) for i in range(n)] and opt.rfa_trace == []
        S.assert_bitwise("raise leaves base", {k: dev[k] for k in base}, S.to_cpu(base))
        # the same optimizer takes the round without the poisoned update afterwards
        rest = [u for i, u in enumerate(ups) if i != bad]
        out = opt.do(dev, _fill([S.to_dev(u, DEV) for u in rest]), total=n - 1)
        w = _check_trace("raise/after", opt, rest, list(range(n - 1)), ("k0", "k1"))
        exp = S.to_cpu(base)
        O.OracleFedAvg().do(exp, _fill([S.to_cpu(u) for u in rest], w), total=1.0)
        S.assert_bitwise("raise/after", {k: out[k] for k in base}, exp)
        return
    out = opt.do(dev, _fill([S.to_dev(u, DEV) for u in ups]), total=n)
    elig = [i for i in range(n) if i != bad]
    w = _check_trace(policy, opt, ups, elig, ("k0", "k1"))
    recs = opt.rfa_records
    assert recs[bad].weight == 0.0 and recs[bad].nonfinite == 1 and math.isnan(recs[bad].dist)
    assert [recs[i].weight for i in elig] == w
    assert (len(opt.update_stats) == n) == (policy == "skip")
    exp = S.to_cpu(base)
    O.OracleFedAvg().do(exp, _fill([S.to_cpu(ups[i]) for i in elig], w), total=1.0)
    S.assert_bitwise(policy, {k: out[k] for k in base}, exp)      # the poisoned update was never read: no inf
    # every update poisoned: None, the base untouched
    for u in ups:
        u["k1"][7] = math.nan
    dev = S.to_dev(base, DEV)
    assert opt.do(dev, _fill([S.to_dev(u, DEV) for u in ups]), total=n) is None
    S.assert_bitwise("all ineligible", {k: dev[k] for k in base}, S.to_cpu(base))


def test_cache_slots_host_residency_and_the_direct_class():
    """The same round from DeviceUpdateCache slab slots, with a host-resident model and pinned
    updates, and through FedGeoMedian: the bits of the plain device round, and the oracle's."""
    from flame_amd.ingest import DeviceUpdateCache
    from flame_amd.optimizer import FedGeoMedian
    O = _oracle()
    n = 9
    g = torch.Generator().manual_seed(23)
    ups = _model(g, n, torch.float32, True)
    base = {"k0": torch.randn(4099, generator=g), "k1": torch.randn(210, generator=g), "nbt": torch.tensor(7)}
    o1 = _drop_in("fedavg", rfa=3)
    hbm = S.to_dev(base, DEV)
    o1.do(hbm, _fill([S.to_dev(u, DEV) for u in ups]), total=n)
    w = _check_trace("plain", o1, ups, list(range(n)), ("k0", "k1"))
    exp = S.to_cpu(base)
    O.OracleFedAvg().do(exp, _fill([S.to_cpu(u) for u in ups], w), total=1.0)
    S.assert_bitwise("plain", {k: hbm[k] for k in base}, exp)
    # slab slots
    cache = DeviceUpdateCache(device=DEV, placement="slab", capacity=n)
    for i, u in enumerate(ups):
        cache[f"e{i:04d}"] = S.TR({k: v.clone() for k, v in u.items()}, 1)
    o2 = FedGeoMedian(iters=3)
    dev = S.to_dev(base, DEV)
    with _Launches() as ln:
        out = o2.do(dev, cache, total=n)
    assert ln.count("flame_update_dist") == 2 and out is dev and len(cache) == 0
    assert o2.rfa_trace == o1.rfa_trace
    S.assert_bitwise("slots", {k: dev[k] for k in base}, exp)
    # host-resident model, pinned updates
    host = {k: v.clone() for k, v in base.items()}
    pinned = [{k: v.clone().pin_memory() for k, v in u.items()} for u in ups]
    before = [{k: v.clone() for k, v in u.items()} for u in pinned]
    o3 = _drop_in("fedavg", rfa=3)
    out = o3.do(host, _fill(pinned), total=n)
    assert out is host and all(not v.is_cuda for v in out.values()) and o3.rfa_trace == o1.rfa_trace
    S.assert_bitwise("host", out, exp)
    for b, a in zip(before, pinned):
        assert all(torch.equal(b[k], a[k]) for k in b), "an update was written"
    # the sharded wrapper's key groups are refused with nothing popped
    cache = _fill([S.to_dev(u, DEV) for u in ups])
    with pytest.raises(NotImplementedError, match="geometric-median"):
        _drop_in("fedavg", rfa=2).do(S.to_dev(base, DEV), cache, total=n, flame_amd_key_groups=[["k0"], ["k1", "nbt"]])
    assert len(cache) == n


# ---------------------------------------------------------------------------- 3. late inputs
def test_late_inputs_on_a_non_default_stream():
    """engine.update_dist and a whole rfa=3 round under tests/stream_case.py: every buffer the
    library reads holds poison until a delay on a non-default stream has passed.  Both entry points
    synchronise by contract (the one D2H of engine._measure), so ``sync=`` names it."""
    import stream_case as SC
    O = _oracle()
    readback = ("engine._measure ends with out.cpu(), the one D2H that waits for the stream "
                "(engine.update_stats / update_dist: 'this is a synchronisation point')")
    n = 9
    g = torch.Generator().manual_seed(47)
    ups = [OrderedDict(u) for u in _model(g, n, torch.float32, True)]
    base0 = OrderedDict([("k0", torch.randn(4099, generator=g)), ("k1", torch.randn(210, generator=g)), ("nbt", torch.tensor(7))])
    z0 = OrderedDict([("k0", torch.randn(4099, generator=g)), ("k1", torch.randn(210, generator=g))])
    ref = R.dist2(ups, z0)[0]
    delay = SC.Delay()
    try:
        def case(L):
            from flame_amd import engine
            opt = _drop_in("fedavg", rfa=3)
            base, srcs, zc = L.weights(base0), [L.weights(u) for u in ups], L.weights(z0)
            with L.stream():
                L.start()
                with L.call("update_dist", sync=readback):
                    d2, nf = engine.update_dist(srcs, zc)
                with L.call("rfa3", sync=readback):
                    out = opt.do(base, _fill([OrderedDict(u) for u in srcs]), total=n)
                L.reuse(*srcs, zc)
                got = L.snap(out)
            L.finish()
            _within("late/update_dist", d2.tolist(), ref, (4099 + 210 + 8) * U53)
            assert not nf.any()
            w = _check_trace("late/rfa3", opt, ups, list(range(n)), ("k0", "k1"))
            exp = OrderedDict((k, v.clone()) for k, v in base0.items())
            O.OracleFedAvg().do(exp, _fill([S.to_cpu(u) for u in ups], w), total=1.0)
            S.assert_bitwise("late/rfa3", got, exp)
            return {"out": got, "d2": {"d": torch.tensor(d2)}, "w": {"w": torch.tensor(w, dtype=torch.float64)}}
        ready = case(SC.Late(delay, ready=True))
        late = case(SC.Late(delay))
        SC.assert_same("rfa3", ready, late)
    finally:
        delay.free()


# ---------------------------------------------------------------------------- 4. the attack
@pytest.mark.parametrize("n,bad", [(9, 3), (33, 12)])
def test_colluders_do_not_move_the_median(n, bad):
    """Honest updates mu + N(0, (2e-3)^2), colluders -4 mu + N(0, (1e-4)^2) (tests/rfa_ref.py's
    attack_round), FedAvg(rfa=5) against plain FedAvg with equal counts: the result is within a
    quarter of plain FedAvg's distance to the honest mean, and the colluders' final weights sum
    below 0.1.  (The fp64 reference alone gives 0.066-0.088 and 0.022-0.032.)"""
    from flame_amd.optimizer import FedAvg
    O = _oracle()
    g = torch.Generator().manual_seed(100 * n)
    ups, pos, honest = R.attack_round(g, n, bad)
    outs = {}
    for name, opt in (("rfa", FedAvg(rfa=5)), ("plain", FedAvg())):
        res = opt.do({"w": torch.zeros(4099, device=DEV)}, _fill([{"w": u.to(DEV)} for u in ups]), total=n)
        outs[name] = res["w"].double().cpu().numpy()
        w = [1.0 / n] * n
        if name == "rfa":
            colluders = math.fsum(opt.rfa_records[i].weight for i in pos)
            assert len(opt.rfa_trace) == 5
            w = [r.weight for r in opt.rfa_records]
        exp = {"w": torch.zeros(4099)}                      # both rounds are the oracle's with their rates
        O.OracleFedAvg().do(exp, _fill([{"w": u.clone()} for u in ups], w), total=1.0)
        S.assert_bitwise(f"attack/{name}", res, exp)
    ratio = np.linalg.norm(outs["rfa"] - honest) / np.linalg.norm(outs["plain"] - honest)
    print(f"n={n} bad={bad}: ratio {ratio:.4f}, colluders' weight {colluders:.4f}")
    assert ratio < 0.25
    assert colluders < 0.1
