"""GPU: trimmed mean / median beyond k = 16 -- flame_agg_select, engine.selected_mean and the
optimizers' ``trim_method`` kwarg.

Every comparison is BITWISE against tests/select_ref.py's ``select`` (the contract of DESIGN.md §2
in numpy / torch-CPU: lo / hi by ``np.sort``, the strictly-inside values added in client order, the
ties at both ends as count x value; a NaN matches any NaN).  Data is N(0, 1) scaled by 2^U(-30, 30)
per value.  On such fp32 / bf16 / f16 data the order of the fp64 adds almost never changes the
rounded result; on f64 it changes nearly half of the elements, so the f64 cases are the ones that
pin the order.  The tests are not marked ``oracle``: the kernel stands outside the launch-branch
table and they consult neither the CPU oracle's counters nor a golden fixture.
"""
import itertools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import scenarios as S
import select_ref as SR
import stream_case as SC
import trimmed_ref as R

pytestmark = [pytest.mark.gpu]

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["f32", "bf16", "f16", "f64"]
NK = [(1, 0), (3, 1), (5, 2), (33, 16), (35, 17), (36, 17), (64, 20), (64, 31), (65, 32), (100, 45), (257, 128)]
SIZES = [(0, 1, 1023), (1024, 1025, 4099)]          # three keys per model; a chunk is 1,024 fp32 elements
BIG_SIZES = (1, 1025)


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
    """``n`` CPU updates + a base over keys of ``sizes`` (generated once per dtype and sizes, grown
    on demand, shared, never modified)."""
    key = (dt, sizes)
    if key not in _BANK:
        g = torch.Generator().manual_seed(2000 + 10 * DTYPES.index(dt) + len(sizes) + sizes[-1])
        _BANK[key] = (g, [], {f"k{j}": _wide(g, s, dt) for j, s in enumerate(sizes)})
    g, ups, base = _BANK[key]
    while len(ups) < n:
        ups.append({f"k{j}": _wide(g, s, dt) for j, s in enumerate(sizes)})
    return ups[:n], base


def _expect(ups, k, base, dt, init_first=False, ref=SR.select):
    return {key: ref([u[key].reshape(-1) for u in ups], k, None if init_first else base[key].reshape(-1), dt)
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
def test_grid_bitwise_against_the_restatement(dt, nk):
    from flame_amd import engine
    n, k = nk
    for sizes in SIZES:
        ups, base = _bank(dt, sizes, n)
        ws = [S.to_dev(w, DEV) for w in ups]
        before = _bytes_of(ws)
        agg = S.to_dev(base, DEV)
        engine.selected_mean(agg, ws, k)
        _check(f"{IDS[DTYPES.index(dt)]} n={n} k={k} {sizes}", agg, _expect(ups, k, base, dt))
        after = _bytes_of(ws)
        assert all(np.array_equal(a[key], b[key]) for a, b in zip(before, after) for key in a), "updates were written"


def test_the_f64_grid_data_pins_the_add_order():
    """Non-vacuity of the claim in the module docstring, on the CPU: at (64, 20) the restatement and
    the ascending sum of the same multiset differ on f64 in a large share of the elements."""
    ups, base = _bank(torch.float64, SIZES[1], 64)
    xs = [u["k2"] for u in ups]
    a, b = SR.select(xs, 20, None, torch.float64), R.by_sort(xs, 20, None, torch.float64)
    differ = int((torch.from_numpy(R.bits(a) != R.bits(b))).sum())
    assert differ > a.numel() // 10, differ


# ---------------------------------------------------------------------------- large n
@pytest.mark.parametrize("nk", [(1025, 100), (1025, 512)], ids=["n1025k100", "n1025k512"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float64], ids=["f32", "bf16", "f64"])
def test_large_n(dt, nk):
    from flame_amd import engine
    n, k = nk
    ups, base = _bank(dt, BIG_SIZES, n)
    agg = S.to_dev(base, DEV)
    engine.selected_mean(agg, [S.to_dev(w, DEV) for w in ups], k)
    _check(f"n={n} k={k}", agg, _expect(ups, k, base, dt))


def test_4096_updates_median():
    from flame_amd import engine
    n, k = 4096, 2047
    assert engine.select_max_clients() >= n
    ups, base = _bank(torch.float32, BIG_SIZES, n)
    agg = S.to_dev(base, DEV)
    engine.selected_mean(agg, [S.to_dev(w, DEV) for w in ups], k)
    _check(f"n={n} k={k}", agg, _expect(ups, k, base, torch.float32))


# ---------------------------------------------------------------------------- placements
@pytest.mark.parametrize("nk", [(64, 31), (35, 17)], ids=["n64k31", "n35k17"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_placements(dt, nk):
    """HBM tensors, UpdateSlab slots (tiled), views one element off alignment (updates and
    aggregate), a host-resident base, init_first; two equal launches give equal bits."""
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
        engine.selected_mean(agg, ws, k)
        _check(f"{layout} n={n} k={k}", agg, exp)
        again = S.to_dev(base, DEV)
        engine.selected_mean(again, ws, k)
        for key in agg:                                   # repeatability: NaN payloads included
            assert np.array_equal(R.bits(agg[key]), R.bits(again[key])), (layout, key)
        first = {key: torch.full_like(v, 7.0) for key, v in agg.items()}
        engine.selected_mean(first, ws, k, init_first=True)
        _check(f"{layout} init_first n={n} k={k}", first, exp_first)
        if layout == "misaligned":                        # a misaligned aggregate as well
            mis = {}
            for key, v in base.items():
                buf = torch.empty(v.numel() + 1, dtype=dt, device=DEV)
                buf[1:].copy_(v)
                mis[key] = buf[1:]
            engine.selected_mean(mis, ws, k)
            _check(f"misaligned aggregate n={n} k={k}", mis, exp)
        del ws, slab
    host = {key: v.clone() for key, v in base.items()}    # host-resident base: staged, written back
    engine.selected_mean(host, [S.to_dev(w, DEV) for w in ups], k)
    assert all(not v.is_cuda for v in host.values())
    _check(f"host base n={n} k={k}", host, exp)


# ---------------------------------------------------------------------------- adversarial columns
def _bits_of(value, dt):
    return int(R.bits(torch.tensor([value], dtype=torch.float64).to(dt))[0])


def _specials(dt):
    """(name, bit pattern): NaN of both signs (a payload bit set), +-inf, subnormals, +-max."""
    ut, _, w, inf = R._U[dt]
    fi = torch.finfo(dt)
    top = 1 << (w - 1)
    return [("+nan", inf | 1), ("-nan", inf | 1 | top), ("+inf", inf), ("-inf", inf | top),
            ("sub", _bits_of(fi.smallest_normal / 4, dt)), ("-sub", _bits_of(-fi.smallest_normal / 8, dt)),
            ("+max", _bits_of(fi.max, dt)), ("-max", _bits_of(fi.min, dt))]


def _adversarial(dt, n, k):
    """``n`` updates of one key as bit patterns [n, numel], every column of the issue's list written
    element by element over N(0, 1) data; returns (tensors, {column name: index})."""
    ut, _, w, _ = R._U[dt]
    wave = 64 * (16 // (w // 8))
    sp = _specials(dt)
    numel = (len(sp) + 3) * wave + 3
    g = torch.Generator().manual_seed(300 + 10 * DTYPES.index(dt) + k)
    bits = np.stack([R.bits(torch.randn(numel, generator=g, dtype=torch.float64).to(dt)) for _ in range(n)]).astype(np.uint64)
    order = torch.randperm(n, generator=g).numpy()       # which client holds the i-th value of a column
    one, two = _bits_of(1.0, dt), _bits_of(2.0, dt)
    top = 1 << (w - 1)
    cols, at = {}, [len(sp) * wave + 7]                   # the structured columns share the waves behind the specials

    def col(name, values):
        c = at[0]
        at[0] += 1
        assert len(values) == n and c < numel
        bits[order, c] = np.asarray(values, np.uint64)
        cols[name] = c

    col("all-equal", [one] * n)
    col("lowest-digit", [one + i for i in range(n)])                              # b, b + 1, .., b + n - 1
    col("lowest-digit-descending", [two + n - 1 - i for i in range(n)])
    col("top-bit", [one | (top if i % 2 else 0) for i in range(n)])               # +-x
    col("top-bit-uneven", [two | (top if i % 3 == 0 else 0) for i in range(n)])
    for c in sorted({max(k - 1, 0), k, k + 1}):                                   # two values, c copies of the smaller
        col(f"two-values-{c}", [one] * c + [two] * (n - c))
        col(f"two-values-neg-{c}", [two | top] * c + [one] * (n - c))
    mid = n - 2 * k                                                               # lo != hi in one last-digit bucket
    col("lo-hi-one-bucket", [_bits_of(0.25, dt)] * k + [one + 1] * (mid // 2 + mid % 2) + [one + 2] * (mid // 2) + [two] * k)
    col("lo-hi-adjacent", [one] * (n // 2) + [one + 1] * (n - n // 2))
    col("low-half-only", [one | (i * 3 + 1) for i in range(n)])                   # f64: the low 32 bits only
    col("high-half-only", [(i + 1) << (w // 2) for i in range(n)])                # f64: the high 32 bits only
    col("high-half-only-neg", [top | ((i + 1) << (w // 2)) for i in range(n)])
    for c in sorted({0, 1, k, k + 1, n // 2, n - k, n}):                          # -0 / +0 mixes
        col(f"zeros-{c}-negative", [top] * c + [0] * (n - c))
    col("zeros-and-ones", [top] * 10 + [0] * 10 + [one] * (n - 20))
    col("max-mixed", [sp[6][1]] * (n // 2) + [sp[7][1]] * (n - n // 2))           # overflows fp32 sums, not fp64
    assert at[0] <= numel
    for i, (name, pattern) in enumerate(sp):              # each special in a wave of its own
        p = i * wave + 5
        for c, holders in enumerate((1, k, k + 1, n - k, n)):
            for u in range(holders):
                bits[(u * 5 + i + c) % n, p + c] = pattern                        # 5 and 64 are coprime: every client once
            cols[f"{name}-{holders}-holders"] = p + c
    return [R.from_bits(bits[i].astype(ut), dt) for i in range(n)], cols


@pytest.mark.parametrize("k", [0, 20, 31])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_adversarial_columns(dt, k):
    from flame_amd import engine
    n = 64
    xs, cols = _adversarial(dt, n, k)
    g = torch.Generator().manual_seed(11)
    base = torch.randn(xs[0].numel(), generator=g).to(dt)
    ws = [{"x": x.to(DEV)} for x in xs]
    for init_first in (False, True):
        agg = {"x": base.to(DEV)}
        engine.selected_mean(agg, ws, k, init_first=init_first)
        exp = SR.select(xs, k, None if init_first else base, dt)
        got = agg["x"].cpu()
        for name, c in cols.items():                      # the named columns first: a failure says which
            R.same_bits(f"{name} k={k} init_first={init_first}", got[c:c + 1], exp[c:c + 1])
        R.same_bits(f"adversarial k={k} init_first={init_first}", got, exp)
        if init_first:
            assert R.bits(got[cols["all-equal"]:cols["all-equal"] + 1])[0] == _bits_of(1.0, dt)
            for name in ("+nan", "-nan", "+inf", "-inf"):
                if k >= 1:                                 # up to k NaN / inf per coordinate vanish ...
                    assert bool(torch.isfinite(got[cols[f"{name}-1-holders"]])), name
                    assert bool(torch.isfinite(got[cols[f"{name}-{k}-holders"]])), name
                assert not bool(torch.isfinite(got[cols[f"{name}-{k + 1}-holders"]])), name     # ... more propagate
                assert not bool(torch.isfinite(got[cols[f"{name}-{n}-holders"]])), name


# ---------------------------------------------------------------------------- against the chain kernel
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_exact_sum_inputs_equal_the_chain_kernel(dt):
    from flame_amd import engine
    g = torch.Generator().manual_seed(15 + DTYPES.index(dt))
    n = 40
    xs = R.exact_inputs(g, dt, n, 2500)
    base = torch.randn(2500, generator=g).to(dt)
    ws = [{"x": x.to(DEV)} for x in xs]
    for k in (0, 1, 8, 16):
        sel, chain = {"x": base.to(DEV)}, {"x": base.to(DEV)}
        engine.selected_mean(sel, ws, k)
        engine.trimmed_mean(chain, ws, k)
        assert np.array_equal(R.bits(sel["x"]), R.bits(chain["x"])), k
        R.same_bits(f"by_sort k={k}", sel["x"], R.by_sort(xs, k, base, dt))


# ---------------------------------------------------------------------------- what the feature buys
def test_31_arbitrary_updates_cannot_move_the_median_out_of_the_honest_range():
    """33 honest N(0, 1) updates and 31 arbitrary ones (all-NaN, +-1e30, sign-flipped honest copies,
    in several arrangements).  Every coordinate of the median (base 0) lies within [min, max] of
    the honest values there and none is NaN; plain FedAvg on the same inputs leaves that range."""
    from flame_amd.optimizer import FedAvg
    g = torch.Generator().manual_seed(19)
    P = 4099
    honest = [torch.randn(P, generator=g) for _ in range(33)]
    lo, hi = torch.stack(honest).min(0).values, torch.stack(honest).max(0).values
    kinds = {"nan": lambda i: torch.full((P,), float("nan")), "+1e30": lambda i: torch.full((P,), 1e30),
             "-1e30": lambda i: torch.full((P,), -1e30), "flip": lambda i: -honest[i]}

    def holds(out):
        out = out.cpu()
        return bool((~torch.isnan(out)).all()) and bool(((out >= lo) & (out <= hi)).all())

    for mix in (("nan",), ("+1e30",), ("-1e30",), ("nan", "+1e30", "-1e30", "flip"), ("+1e30", "-1e30"), ("flip", "nan")):
        bad = [kinds[mix[i % len(mix)]](i) for i in range(31)]
        ups = list(itertools.chain.from_iterable(zip(honest, bad))) + honest[31:]        # interleaved: 64 updates
        assert len(ups) == 64
        outs = {}
        for name, opt in (("median", FedAvg(trim="median", trim_method="select")), ("plain", FedAvg())):
            cache = S.SortedCache()
            for i, u in enumerate(ups):
                cache[f"e{i:02d}"] = S.TR({"w": u.to(DEV)}, 1)
            outs[name] = opt.do({"w": torch.zeros(P, device=DEV)}, cache, total=64)["w"]
        assert holds(outs["median"]), mix
        assert not holds(outs["plain"]), mix
        R.same_bits(f"robust {mix}", outs["median"], SR.select(ups, 31, torch.zeros(P), torch.float32))


# ---------------------------------------------------------------------------- the public surface
class _MC:
    def __init__(self):
        self.saved = []

    def save(self, mtype, alias, value):
        self.saved.append((mtype, alias, value))


def _surface_model(g, i):
    return {"w": _wide(g, 4099, torch.float32), "h": _wide(g, 3 * 2048 + 5, torch.bfloat16).view(-1, 1),
            "d": _wide(g, 1025, torch.float64), "nbt": torch.tensor(100 + 37 * i)}


SURFACE_DTYPES = (("w", torch.float32), ("h", torch.bfloat16), ("d", torch.float64))


@pytest.mark.parametrize("case", ["fedavg", "fedprox", "fedmedian"])
def test_optimizers_over_a_device_update_cache(case):
    """do() over a DeviceUpdateCache (slab) of 64 updates: float keys equal the restatement, the
    int64 ``num_batches_tracked`` equals the reference's FedAvg statement with rate 1 / n in
    torch-CPU ops, the cache is drained, the slab's bytes are unchanged, the records are kept."""
    from flame_amd.ingest import DeviceUpdateCache
    from flame_amd.optimizer import FedAvg, FedMedian, FedProx
    n, k = 64, 31
    opt = {"fedavg": FedAvg(trim="median", trim_method="select"), "fedprox": FedProx(mu=0.1, trim="median", trim_method="select"),
           "fedmedian": FedMedian(trim_method="select")}[case]
    opt.metric_collector = mc = _MC()
    g = torch.Generator().manual_seed(50)
    base = _surface_model(g, 0)
    ups = [_surface_model(g, 1 + i) for i in range(n)]
    cache = DeviceUpdateCache(device=DEV, placement="slab", capacity=n)
    for i, u in enumerate(ups):
        cache[f"e{i:02d}"] = S.TR({key: v.clone() for key, v in u.items()}, 3 + i)
    assert cache.slab is not None
    slab_before = {dt: st.clone() for dt, st in cache.slab.storage.items()}
    dev = S.to_dev(base, DEV)
    out = opt.do(dev, cache, total=sum(3 + i for i in range(n)))
    assert out is dev and len(cache) == 0 and opt.trim_k == k and opt.trim_kernel == "select"
    for key, dt in SURFACE_DTYPES:
        R.same_bits(f"{case}/{key}", out[key], SR.select([u[key].reshape(-1) for u in ups], k, base[key].reshape(-1), dt))
        assert out[key].shape == base[key].shape
    nbt = base["nbt"].clone()
    for u in ups:                                         # fedavg.py:93-104 with rate = 1 / n
        nbt += (u["nbt"] * (1.0 / n)).to(u["nbt"].dtype)
    assert out["nbt"].dtype == torch.int64 and int(out["nbt"]) == int(nbt)
    for dt, st in cache.slab.storage.items():
        assert torch.equal(st.view(torch.uint8), slab_before[dt].view(torch.uint8)), "the slab was written"
    alias = type(opt).__name__.lower()
    for m in (("trim_k", alias, k), ("updates_trimmed_from", alias, n), ("trim_kernel", alias, "select")):
        assert m in mc.saved, m


def test_fedmedian_over_1025_updates():
    from flame_amd.optimizer import FedMedian
    n = 1025
    ups, base = _bank(torch.float64, BIG_SIZES, n)
    cache = S.SortedCache()
    for i, u in enumerate(ups):
        cache[f"e{i:04d}"] = S.TR(S.to_dev(u, DEV), 1)
    opt = FedMedian(trim_method="select")
    out = opt.do(S.to_dev(base, DEV), cache, total=n)
    assert opt.trim_k == 512 and opt.trim_kernel == "select" and len(cache) == 0
    _check("fedmedian n=1025", out, _expect(ups, 512, base, torch.float64))


def test_nonfinite_skip_drops_an_all_nan_update_first():
    from flame_amd.optimizer import FedAvg
    n = 64
    g = torch.Generator().manual_seed(51)
    base = _surface_model(g, 0)
    ups = [_surface_model(g, 1 + i) for i in range(n)]
    ups[5] = {key: (torch.full_like(v, float("nan")) if v.is_floating_point() else v) for key, v in ups[5].items()}
    cache = S.SortedCache()
    for i, u in enumerate(ups):
        cache[f"e{i:02d}"] = S.TR(S.to_dev(u, DEV), 1)
    opt = FedAvg(trim="median", trim_method="select", nonfinite="skip")
    opt.metric_collector = mc = _MC()
    out = opt.do(S.to_dev(base, DEV), cache, total=n)
    rest = [u for i, u in enumerate(ups) if i != 5]
    assert [r.skipped for r in opt.update_stats] == [i == 5 for i in range(n)] and opt.trim_k == 31 and len(cache) == 0
    for key, dt in SURFACE_DTYPES:
        R.same_bits(f"skip/{key}", out[key], SR.select([u[key].reshape(-1) for u in rest], 31, base[key].reshape(-1), dt))
    assert ("updates_trimmed_from", "fedavg", 63) in mc.saved and ("updates_skipped", "fedavg", 1) in mc.saved


def test_auto_takes_the_chain_at_34_updates_and_the_selection_at_35():
    from flame_amd.optimizer import FedAvg
    g = torch.Generator().manual_seed(52)
    base = _surface_model(g, 0)
    ups = [_surface_model(g, 1 + i) for i in range(35)]
    for n, k, kernel, ref in ((34, 16, "chain", R.stream), (35, 17, "select", SR.select)):
        cache = S.SortedCache()
        for i, u in enumerate(ups[:n]):
            cache[f"e{i:02d}"] = S.TR(S.to_dev(u, DEV), 1)
        opt = FedAvg(trim="median", trim_method="auto")
        out = opt.do(S.to_dev(base, DEV), cache, total=n)
        assert opt.trim_k == k and opt.trim_kernel == kernel
        for key, dt in SURFACE_DTYPES:
            R.same_bits(f"auto n={n}/{key}", out[key], ref([u[key].reshape(-1) for u in ups[:n]], k, base[key].reshape(-1), dt))


def test_launch_branch_table_is_unchanged_by_select_launches():
    from flame_amd import _native, engine
    before = _native.launch_branch_counts()
    assert len(before) == 100
    agg = {"x": torch.zeros(100, device=DEV)}
    engine.selected_mean(agg, [{"x": torch.full((100,), float(i), device=DEV)} for i in range(41)], 19)
    assert agg["x"].cpu().tolist() == [20.0] * 100                # the mean of 19, 20, 21
    assert _native.launch_branch_counts() == before


# ---------------------------------------------------------------------------- a non-default stream, late inputs
@pytest.fixture(scope="module")
def delay():
    d = SC.Delay()
    yield d
    d.free()


def test_median_of_35_late_updates_on_a_stream_of_its_own(delay):
    """tests/stream_case.py's case: every buffer holds poison until a delay on the caller's stream
    has run; the selection kernel must be ordered behind it (asynchronous: nothing is read back)."""
    from flame_amd.optimizer import FedMedian
    n, k = 35, 17
    g = torch.Generator().manual_seed(53)
    spec = (("w", torch.float32, 4099), ("d", torch.float64, 1025))
    base0 = OrderedDict((key, _wide(g, numel, dt)) for key, dt, numel in spec)
    ups = [OrderedDict((key, _wide(g, numel, dt)) for key, dt, numel in spec) for _ in range(n)]
    exp = {key: SR.select([u[key] for u in ups], k, base0[key], dt) for key, dt, _ in spec}

    def case(L):
        opt = FedMedian(trim_method="select")
        base, srcs = L.weights(base0), [L.weights(u) for u in ups]
        with L.stream():
            L.start()
            cache = S.SortedCache()
            for i, u in enumerate(srcs):
                cache[f"e{i:02d}"] = S.TR(OrderedDict(u), 1)
            with L.call("median35"):
                out = opt.do(base, cache, total=n)
            L.reuse(*srcs)
            got = L.snap(out)
        L.finish()
        assert opt.trim_k == k and opt.trim_kernel == "select" and out is base
        for key in exp:
            R.same_bits(f"median35/{key}", got[key], exp[key])
        return {"out": got}
    ready = case(SC.Late(delay, ready=True))
    late = case(SC.Late(delay))
    SC.assert_same("median35", ready, late)
