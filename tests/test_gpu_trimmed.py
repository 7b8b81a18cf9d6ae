"""GPU: coordinate-wise trimmed mean / median -- flame_agg_trimmed, engine.trimmed_mean and the
optimizers' ``trim`` kwarg.

Every comparison is BITWISE against tests/trimmed_ref.py's ``stream`` (the streaming selection of
DESIGN.md §2 in numpy / torch-CPU; a NaN matches any NaN, sign and payload are not pinned), on
data N(0, 1) scaled by 2^U(-30, 30) per value so that the order the kept values are added in
matters.  On exact-sum inputs the kernel also equals the sort-based definition (``by_sort``,
``torch.sort``).  The tests are not marked ``oracle``: the kernel stands outside the launch-branch
table and they consult neither the CPU oracle's counters nor a golden fixture.
"""
import itertools

import numpy as np
import pytest
import torch

import scenarios as S
import trimmed_ref as R

pytestmark = [pytest.mark.gpu]

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["f32", "bf16", "f16", "f64"]
# each chain capacity (1, 2, 3, 4, 6, 8, 12, 16) at its top and just above the one below; the
# client-unroll boundaries at 4 / 5 and 8 / 9 arrivals of a phase
NK = [(1, 0), (3, 1), (5, 2), (8, 1), (9, 1), (9, 4), (17, 8), (33, 16), (40, 3), (70, 8),
      (11, 5), (13, 6), (15, 7), (19, 9), (25, 12), (27, 13), (34, 16), (4, 0)]
SIZES = [(0, 1, 1023), (1024, 1025, 4099)]          # three keys per model; a chunk is 1,024 fp32 elements


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()


def _wide(g, numel, dt):
    """N(0, 1) * 2^U(-30, 30) per value, in ``dt`` (fp16 saturates some to +-inf / 0: still data)."""
    x = torch.randn(numel, generator=g, dtype=torch.float64)
    e = torch.rand(numel, generator=g, dtype=torch.float64) * 60 - 30
    return (x * torch.exp2(e)).to(dt)


_BANK = {}


def _bank(dt, sizes, n):
    """``n`` CPU updates + a base over keys of ``sizes`` (generated once per dtype and sizes, shared,
    never modified)."""
    key = (dt, sizes)
    if key not in _BANK:
        g = torch.Generator().manual_seed(1000 + 10 * DTYPES.index(dt) + len(sizes) + sizes[-1])
        ups = [{f"k{j}": _wide(g, s, dt) for j, s in enumerate(sizes)} for _ in range(70)]
        base = {f"k{j}": _wide(g, s, dt) for j, s in enumerate(sizes)}
        _BANK[key] = (ups, base)
    ups, base = _BANK[key]
    return ups[:n], base


def _expect(ups, k, base, dt, init_first=False):
    return {key: R.stream([u[key].reshape(-1) for u in ups], k, None if init_first else base[key].reshape(-1), dt)
            .view(base[key].shape) for key in base}


def _check(label, got, exp):
    assert list(got.keys()) == list(exp.keys()), label
    for key in exp:
        assert got[key].shape == exp[key].shape, (label, key)
        R.same_bits(f"{label}/{key}", got[key], exp[key])


def _bytes_of(ws):
    return [{k: R.bits(w[k]) for k in w.keys() if w[k].is_floating_point()} for w in ws]


def _layout(ups, layout):
    """The same updates on the GPU as plain tensors, UpdateSlab slots (tiled), or views one element
    off 16-byte alignment (the scalar path)."""
    if layout == "tensors":
        return [S.to_dev(w, DEV) for w in ups], None
    if layout == "misaligned":
        out = []
        for w in ups:
            d = {}
            for k, v in w.items():
                buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=DEV)
                buf[1:].copy_(v.reshape(-1))
                d[k] = buf[1:].view(v.shape)
                assert v.numel() == 0 or d[k].data_ptr() % 16 != 0
            out.append(d)
        return out, None
    from flame_amd.slab import UpdateSlab
    slab = UpdateSlab(ups[0], len(ups), DEV)
    return [slab.put(S.to_dev(w, DEV)) for w in ups], slab


# ---------------------------------------------------------------------------- the main grid
@pytest.mark.parametrize("nk", NK, ids=[f"n{n}k{k}" for n, k in NK])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_grid_bitwise_against_the_stream(dt, nk):
    from flame_amd import engine
    n, k = nk
    for sizes in SIZES:
        ups, base = _bank(dt, sizes, n)
        ws = [S.to_dev(w, DEV) for w in ups]
        before = _bytes_of(ws)
        agg = S.to_dev(base, DEV)
        engine.trimmed_mean(agg, ws, k)
        _check(f"{IDS[DTYPES.index(dt)]} n={n} k={k} {sizes}", agg, _expect(ups, k, base, dt))
        after = _bytes_of(ws)
        assert all(np.array_equal(a[key], b[key]) for a, b in zip(before, after) for key in a), "updates were written"


# ---------------------------------------------------------------------------- placements
@pytest.mark.parametrize("nk", [(9, 2), (33, 16)], ids=["n9k2", "n33k16"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_placements(dt, nk):
    """HBM tensors, UpdateSlab slots (tiled), views one element off alignment, a host-resident
    base, init_first; two equal launches give equal bits."""
    from flame_amd import engine
    n, k = nk
    sizes = SIZES[1]
    ups, base = _bank(dt, sizes, n)
    exp = _expect(ups, k, base, dt)
    exp_first = _expect(ups, k, base, dt, init_first=True)
    for layout in ("tensors", "slab", "misaligned"):
        ws, slab = _layout(ups, layout)
        if layout == "slab":
            assert engine.tiled_stride(ws[0]["k2"], sizes[2])
        agg = S.to_dev(base, DEV)
        engine.trimmed_mean(agg, ws, k)
        _check(f"{layout} n={n} k={k}", agg, exp)
        again = S.to_dev(base, DEV)
        engine.trimmed_mean(again, ws, k)
        for key in agg:                                   # repeatability: NaN payloads included
            assert np.array_equal(R.bits(agg[key]), R.bits(again[key])), (layout, key)
        first = {key: torch.full_like(v, 7.0) for key, v in agg.items()}
        engine.trimmed_mean(first, ws, k, init_first=True)
        _check(f"{layout} init_first n={n} k={k}", first, exp_first)
        if layout == "misaligned":                        # a misaligned aggregate as well
            mis = {}
            for key, v in base.items():
                buf = torch.empty(v.numel() + 1, dtype=dt, device=DEV)
                buf[1:].copy_(v)
                mis[key] = buf[1:]
            engine.trimmed_mean(mis, ws, k)
            _check(f"misaligned aggregate n={n} k={k}", mis, exp)
        del ws, slab
    host = {key: v.clone() for key, v in base.items()}    # host-resident base: staged, written back
    engine.trimmed_mean(host, [S.to_dev(w, DEV) for w in ups], k)
    assert all(not v.is_cuda for v in host.values())
    _check(f"host base n={n} k={k}", host, exp)


# ---------------------------------------------------------------------------- special values
def _specials(dt):
    fi = torch.finfo(dt)
    pnan = R.from_bits(np.array([R._U[dt][3] | 1], R._U[dt][0]), dt)[0]                      # +NaN, a payload bit
    nnan = R.from_bits(np.array([R._U[dt][3] | 1 | (1 << (R._U[dt][2] - 1))], R._U[dt][0]), dt)[0]   # -NaN
    assert bool(torch.isnan(pnan)) and bool(torch.isnan(nnan))
    return [("+nan", pnan), ("-nan", nnan), ("+inf", torch.tensor(float("inf"), dtype=dt)),
            ("-inf", torch.tensor(float("-inf"), dtype=dt)), ("-0", torch.tensor(-0.0, dtype=dt)),
            ("+0", torch.tensor(0.0, dtype=dt)), ("sub", torch.tensor(fi.smallest_normal, dtype=torch.float64).div(4).to(dt)),
            ("-sub", torch.tensor(-fi.smallest_normal, dtype=torch.float64).div(8).to(dt)),
            ("+max", torch.tensor(fi.max, dtype=dt)), ("-max", torch.tensor(fi.min, dtype=dt))]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_special_values_at_the_k_boundary(dt):
    """(n, k) = (9, 2).  Each special value is planted in a wave of its own (64 lanes x one 16-byte
    vector), at coordinates where exactly 1, k, k + 1, n - k and all n updates hold it; +-0 are also
    mixed over all updates (the sign of an all-zero kept set follows the restatement: the sum starts
    at +0.0) and +max / -max share coordinates (their sum overflows fp32, not fp64).  With a base
    and with init_first, as tensors and on the scalar path."""
    from flame_amd import engine
    n, k = 9, 2
    wave = 64 * (16 // torch.empty((), dtype=dt).element_size())
    sp = _specials(dt)
    numel = (len(sp) + 2) * wave + 3
    g = torch.Generator().manual_seed(77 + DTYPES.index(dt))
    xs = [torch.randn(numel, generator=g).to(dt) for _ in range(n)]
    for i, (_, v) in enumerate(sp):
        p = i * wave + 5
        for c, holders in enumerate((1, k, k + 1, n - k, n)):
            for u in range(holders):
                xs[(u * 4 + i + c) % n][p + c] = v                 # u * 4 mod 9 visits every client once
    p = len(sp) * wave + 9                                         # +-0 mixed over all updates; +-max mixed
    for u in range(n):
        xs[u][p] = -0.0 if u % 2 else 0.0
        xs[u][p + 1] = -0.0
        xs[u][p + 2] = torch.finfo(dt).max if u < 5 else torch.finfo(dt).min
        xs[u][p + 3] = torch.finfo(dt).max if u != 4 else 1.0
    ups = [{"x": x} for x in xs]
    base = {"x": torch.randn(numel, generator=g).to(dt)}
    base["x"][p:p + 2] = -0.0
    for layout in ("tensors", "misaligned"):
        ws, _ = _layout(ups, layout)
        for init_first in (False, True):
            agg = S.to_dev(base, DEV)
            engine.trimmed_mean(agg, ws, k, init_first=init_first)
            exp = _expect(ups, k, base, dt, init_first)
            _check(f"special/{layout}/init_first={init_first}", agg, exp)
            got = agg["x"].cpu()
            if init_first:
                for i, (name, _) in enumerate(sp[:4]):             # up to k NaN / inf per coordinate vanish ...
                    q = i * wave + 5
                    assert bool(torch.isfinite(got[q:q + 2]).all()), name
                    assert not bool(torch.isfinite(got[q + 2:q + 5]).any()), name    # ... more of them propagate
                assert R.bits(got[p:p + 2]).tolist() == [0, 0]                       # +0.0 + (-0.0) ... = +0.0
                if dt != torch.float64:
                    assert bool(torch.isfinite(got[p + 2:p + 4]).all()) and float(got[p + 3]) == torch.finfo(dt).max


# ---------------------------------------------------------------------------- against the definition
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_exact_sum_inputs_equal_the_sorted_definition(dt):
    from flame_amd import engine
    g = torch.Generator().manual_seed(5 + DTYPES.index(dt))
    for n, k in [(9, 2), (33, 16), (70, 8), (8, 3), (7, 0)]:
        xs = R.exact_inputs(g, dt, n, 2500)
        base = torch.randn(2500, generator=g).to(dt)
        agg = {"x": base.to(DEV)}
        engine.trimmed_mean(agg, [{"x": x.to(DEV)} for x in xs], k)
        R.same_bits(f"by_sort n={n} k={k}", agg["x"], R.by_sort(xs, k, base, dt))
        if dt == torch.float32:
            kept = torch.sort(torch.stack(xs), 0).values[k:n - k].double()
            acc = torch.zeros(2500, dtype=torch.float64)
            for row in kept:
                acc = acc + row
            R.same_bits(f"torch.sort n={n} k={k}", agg["x"], base + (acc / (n - 2 * k)).float())


# ---------------------------------------------------------------------------- what the feature buys
def test_two_arbitrary_updates_cannot_move_a_coordinate_out_of_the_honest_range():
    """n = 9, k = 2: 7 honest N(0, 1) updates and 2 arbitrary ones (every combination of all-NaN,
    1e30, -1e30 and a sign-flipped copy of an honest update).  Every trimmed coordinate (base 0)
    lies within [min, max] of the honest values there and none is NaN; plain FedAvg on the same
    inputs breaks that for every combination."""
    from flame_amd.optimizer import FedAvg
    g = torch.Generator().manual_seed(9)
    P = 4099
    honest = [torch.randn(P, generator=g) for _ in range(7)]
    lo, hi = torch.stack(honest).min(0).values, torch.stack(honest).max(0).values
    bad = {"nan": torch.full((P,), float("nan")), "+1e30": torch.full((P,), 1e30), "-1e30": torch.full((P,), -1e30),
           "flip": -honest[3]}

    def holds(out):
        out = out.cpu()
        return bool((~torch.isnan(out)).all()) and bool(((out >= lo) & (out <= hi)).all())

    for a, b in itertools.product(bad, bad):
        ups = honest[:2] + [bad[a]] + honest[2:6] + [bad[b]] + honest[6:]
        outs = {}
        for name, opt in (("trim", FedAvg(trim=2)), ("plain", FedAvg())):
            cache = S.SortedCache()
            for i, u in enumerate(ups):
                cache[f"e{i}"] = S.TR({"w": u.to(DEV)}, 1)
            outs[name] = opt.do({"w": torch.zeros(P, device=DEV)}, cache, total=9)["w"]
        assert holds(outs["trim"]), (a, b)
        assert not holds(outs["plain"]), (a, b)
        R.same_bits(f"robust {a},{b}", outs["trim"], R.stream(ups, 2, torch.zeros(P), torch.float32))


# ---------------------------------------------------------------------------- the public surface
class _MC:
    def __init__(self):
        self.saved = []

    def save(self, mtype, alias, value):
        self.saved.append((mtype, alias, value))


def _surface_model(g, i):
    return {"w": _wide(g, 4099, torch.float32), "h": _wide(g, 3 * 2048 + 5, torch.bfloat16).view(-1, 1),
            "nbt": torch.tensor(100 + 37 * i)}


@pytest.mark.parametrize("case", ["fedavg-int", "fedavg-fraction", "fedmedian", "fedprox"])
def test_optimizers_over_a_device_update_cache(case):
    """do() over a DeviceUpdateCache (slab): float keys equal the restatement, the int64
    ``num_batches_tracked`` equals the reference's FedAvg statement with rate 1 / n in torch-CPU
    ops, the cache is drained, the slab's bytes are unchanged and the metrics are recorded."""
    from flame_amd.ingest import DeviceUpdateCache
    from flame_amd.optimizer import FedAvg, FedMedian, FedProx
    n = 9
    opt, k = {"fedavg-int": (FedAvg(trim=2), 2), "fedavg-fraction": (FedAvg(trim=0.25), 2),
              "fedmedian": (FedMedian(), 4), "fedprox": (FedProx(mu=0.1, trim=1), 1)}[case]
    opt.metric_collector = mc = _MC()
    g = torch.Generator().manual_seed(40)
    base = _surface_model(g, 0)
    ups = [_surface_model(g, 1 + i) for i in range(n)]
    cache = DeviceUpdateCache(device=DEV, placement="slab", capacity=n)
    for i, u in enumerate(ups):
        cache[f"e{i:02d}"] = S.TR({key: v.clone() for key, v in u.items()}, 3 + i)
    assert cache.slab is not None
    slab_before = {dt: st.clone() for dt, st in cache.slab.storage.items()}
    dev = S.to_dev(base, DEV)
    out = opt.do(dev, cache, total=sum(3 + i for i in range(n)))
    assert out is dev and len(cache) == 0 and opt.trim_k == k
    for key, dt in (("w", torch.float32), ("h", torch.bfloat16)):
        R.same_bits(f"{case}/{key}", out[key], R.stream([u[key].reshape(-1) for u in ups], k, base[key].reshape(-1), dt))
        assert out[key].shape == base[key].shape
    nbt = base["nbt"].clone()
    for u in ups:                                         # fedavg.py:93-104 with rate = 1 / n
        nbt += (u["nbt"] * (1.0 / n)).to(u["nbt"].dtype)
    assert out["nbt"].dtype == torch.int64 and int(out["nbt"]) == int(nbt)
    for dt, st in cache.slab.storage.items():
        assert torch.equal(st.view(torch.uint8), slab_before[dt].view(torch.uint8)), "the slab was written"
    alias = type(opt).__name__.lower()
    assert ("trim_k", alias, k) in mc.saved and ("updates_trimmed_from", alias, n) in mc.saved


def test_nonfinite_skip_drops_an_all_nan_update_first():
    from flame_amd.ingest import DeviceUpdateCache
    from flame_amd.optimizer import FedAvg
    n = 9
    g = torch.Generator().manual_seed(41)
    base = _surface_model(g, 0)
    ups = [_surface_model(g, 1 + i) for i in range(n)]
    ups[5] = {key: (torch.full_like(v, float("nan")) if v.is_floating_point() else v) for key, v in ups[5].items()}
    cache = DeviceUpdateCache(device=DEV, placement="slab", capacity=n)
    for i, u in enumerate(ups):
        cache[f"e{i:02d}"] = S.TR({key: v.clone() for key, v in u.items()}, 1)
    opt = FedAvg(trim=0.25, nonfinite="skip")
    opt.metric_collector = mc = _MC()
    dev = S.to_dev(base, DEV)
    out = opt.do(dev, cache, total=n)
    rest = [u for i, u in enumerate(ups) if i != 5]
    assert [r.skipped for r in opt.update_stats] == [i == 5 for i in range(n)] and opt.trim_k == 2 and len(cache) == 0
    for key, dt in (("w", torch.float32), ("h", torch.bfloat16)):
        R.same_bits(f"skip/{key}", out[key], R.stream([u[key].reshape(-1) for u in rest], 2, base[key].reshape(-1), dt))
    assert ("updates_trimmed_from", "fedavg", 8) in mc.saved and ("updates_skipped", "fedavg", 1) in mc.saved


def test_launch_branch_table_is_unchanged_by_trimmed_launches():
    from flame_amd import _native, engine
    before = _native.launch_branch_counts()
    assert len(before) == 100
    agg = {"x": torch.zeros(100, device=DEV)}
    engine.trimmed_mean(agg, [{"x": torch.full((100,), float(i), device=DEV)} for i in range(5)], 1)
    assert agg["x"].cpu().tolist() == [2.0] * 100                 # the mean of 1, 2, 3
    assert _native.launch_branch_counts() == before
