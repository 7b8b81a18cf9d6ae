"""GPU: the server-side update guard -- flame_update_stats, flame_agg_reduce_scaled, and the
optimizers' ``clip_threshold`` / ``nonfinite`` kwargs.

* Statistics: ``sumsq`` against ``math.fsum`` of the fp64 squares (correctly rounded), relative
  error <= (n + 1) * 2^-53 with n the update's float element count -- Higham's bound for a sum of
  n non-negative terms in ANY order (each of the n - 1 additions is off by at most 2^-53
  relative, first-order, plus the reference's own rounding), derived, not measured.  ``nonfinite``
  exact.  Two equal launches give equal bits.
* Scaled reduction: bitwise against ``oracle.reduce_tensor`` on CPU updates pre-scaled with
  ``oracle.tmp_tensor(v, scale)`` -- the reference's two statements (differential_privacy.py:79-82,
  fedavg.py:93-104).
* Optimizers: the reported scales rebuild the expected model with the oracle as above.

Every test consults the CPU oracle (or the golden fixture), so the branches they reach are credited.
"""
import math

import numpy as np
import pytest
import torch

import scenarios as S

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DEV = "cuda:0"
U53 = 2.0 ** -53
SIZES = [1023, 0, 1, 3, 1024, 4099, 70001]      # several keys per model, an empty one among them
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["f32", "bf16", "f16", "f64"]
LAYOUTS = ["tensors", "slab", "misaligned"]
# a product of one of these with an ordinary value is subnormal in the dtype
TINY = {torch.float32: 1e-41, torch.bfloat16: 1e-40, torch.float16: 3e-7, torch.float64: 1e-310}


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()


def _oracle():
    from oracle import oracle as O
    return O


_BANK = {}


def _bank(dt, n):
    """``n`` CPU updates of dtype ``dt`` over SIZES (generated once per dtype, shared, never
    modified) and each one's exact sum of squares."""
    if dt not in _BANK:
        g = torch.Generator().manual_seed(100 + DTYPES.index(dt))
        ups, exact = [], []
        for i in range(150):
            w = {f"k{j}": (torch.randn(s, generator=g) * (0.5 + 0.01 * i)).to(dt) for j, s in enumerate(SIZES)}
            ups.append(w)
            exact.append(_fsum_sq(w.values()))
        _BANK[dt] = (ups, exact)
    ups, exact = _BANK[dt]
    return ups[:n], exact[:n]


def _fsum_sq(tensors):
    """fsum of the fp64 squares of every finite float element: correctly rounded."""
    terms = []
    for t in tensors:
        if not t.is_floating_point():
            continue
        x = t.detach().cpu().double().reshape(-1)
        x = x[torch.isfinite(x)]
        terms.extend((x * x).tolist())
    return math.fsum(terms)


def _layout(ups, layout):
    """The same updates on the GPU as plain tensors, UpdateSlab slots, or views one element
    off 16-byte alignment."""
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


def _check_stats(label, sumsq, nonfinite, exact, n_elems, want_nf):
    for i, (got, ref) in enumerate(zip(sumsq, exact)):
        tol = (n_elems + 1) * U53
        err = abs(got - ref) / ref if ref else abs(got)
        print(f"{label} client {i}: sumsq rel err {err:.3e} (bound {tol:.3e})")
        assert err <= tol, f"{label} client {i}: {got!r} vs fsum {ref!r}: rel {err:.3e} > {tol:.3e}"
    assert [int(x) for x in nonfinite] == list(want_nf), label


def _scales_for(dt, n):
    base = [1.0, 0.37, TINY[dt], 0.9990234375, 1.0, 0.5, 1e-3, 0.73, 0.123456789]
    return [base[i % len(base)] for i in range(n)]


def _expected_reduce(O, base, ups, rates, scales, init_first):
    exp = {}
    for k, b in base.items():
        acc = b.clone()
        pre = [O.tmp_tensor(w[k], s) for w, s in zip(ups, scales)]          # torch.mul(d_w, scale)
        if init_first:          # acc = tmp_0 (the oracle's init_first keeps the call's LAST client)
            O.reduce_tensor(acc, pre[:1], rates[:1], init_first=True)
            O.reduce_tensor(acc, pre[1:], rates[1:])
        else:
            O.reduce_tensor(acc, pre, rates)                                # fedavg.py:93-104
        exp[k] = acc
    return exp


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stats_and_scaled_reduce(dt, layout):
    """Per dtype x layout, for 1 / 8 / 9 / 150 clients (150: more than one batch of the statistics
    kernel's client loop, whole client groups and clients left over): sumsq, nonfinite,
    repeatability, then the scaled reduction from a base and INIT_FIRST, and the all-ones case
    against the plain kernel."""
    from flame_amd import engine
    O = _oracle()
    for n in (1, 8, 9, 150):
        ups, exact = _bank(dt, n)
        ws, slab = _layout(ups, layout)
        label = f"{IDS[DTYPES.index(dt)]}/{layout}/{n}"
        sumsq, nf = engine.update_stats(ws, DEV)
        assert sumsq.dtype == np.float64 and nf.dtype == np.int64 and sumsq.shape == nf.shape == (n,)
        _check_stats(label, sumsq, nf, exact, sum(SIZES), [0] * n)
        again, nf2 = engine.update_stats(ws, DEV)
        assert np.array_equal(sumsq.view(np.uint64), again.view(np.uint64)) and np.array_equal(nf, nf2), label
        # scaled reduction
        g = torch.Generator().manual_seed(n)
        base = {k: torch.randn(v.shape, generator=g).to(dt) for k, v in ups[0].items()}
        counts = [3 + (7 * i) % 11 for i in range(n)]
        rates = [c / sum(counts) for c in counts]
        scales = _scales_for(dt, n)
        keys = list(base.keys())
        for init_first in (False, True):
            outs = [base[k].to(DEV) for k in keys]
            engine.reduce_(outs, None if init_first else outs, [[w[k] for w in ws] for k in keys], rates,
                           init_first=init_first, scales=scales)
            exp = _expected_reduce(O, base, ups, rates, scales, init_first)
            S.assert_bitwise(f"{label}/init_first={init_first}", dict(zip(keys, outs)), exp)
        ones = [base[k].to(DEV) for k in keys]
        engine.reduce_(ones, ones, [[w[k] for w in ws] for k in keys], rates, scales=[1.0] * n)
        plain = [base[k].to(DEV) for k in keys]
        engine.reduce_(plain, plain, [[w[k] for w in ws] for k in keys], rates)
        S.assert_bitwise(f"{label}/ones", dict(zip(keys, ones)), {k: p.cpu() for k, p in zip(keys, plain)})
        del ws, slab


def test_stats_two_dtype_model_and_ignored_keys():
    """A model of f32 and bf16 keys (two launches accumulate into one output) with an int64 0-dim
    key and a bool mask, which take no part; as tensors and as slab slots."""
    from flame_amd import engine
    from flame_amd.ingest import DeviceUpdateCache
    O = _oracle()
    g = torch.Generator().manual_seed(5)
    ups = []
    for i in range(9):
        ups.append({"a": torch.randn(4099, generator=g), "nbt": torch.tensor(7 + i),
                    "b": torch.randn(3 * 2048 + 5, generator=g).bfloat16(), "mask": torch.rand(33, generator=g) > 0.5,
                    "c": torch.randn(17, 3, generator=g)})
    exact = [_fsum_sq(w.values()) for w in ups]
    n_el = 4099 + 3 * 2048 + 5 + 51
    sumsq, nf = engine.update_stats([S.to_dev(w, DEV) for w in ups], DEV)
    _check_stats("two-dtype/tensors", sumsq, nf, exact, n_el, [0] * 9)
    cache = DeviceUpdateCache(device=DEV, placement="slab", capacity=9)
    for i, w in enumerate(ups):
        cache[f"e{i}"] = S.TR({k: v.clone() for k, v in w.items()}, 1)
    ws = [cache[f"e{i}"].weights for i in range(9)]
    sumsq2, nf2 = engine.update_stats(ws, DEV)
    _check_stats("two-dtype/slab", sumsq2, nf2, exact, n_el, [0] * 9)
    # the guard's scale for these (consults the oracle: a clipped f32 key through the scaled kernel)
    scales = [min(1.0, 50.0 / (math.sqrt(s) + 1e-6)) for s in exact]
    out = torch.zeros(4099, device=DEV)
    engine.reduce_([out], [out], [[w["a"].to(DEV) for w in ups]], [1 / 9] * 9, scales=scales)
    exp = torch.zeros(4099)
    O.reduce_tensor(exp, [O.tmp_tensor(w["a"], s) for w, s in zip(ups, scales)], [1 / 9] * 9)
    S.assert_bitwise("two-dtype/scaled", {"a": out}, {"a": exp})


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stats_special_values(dt):
    """NaN, +-inf, subnormals, +-0, the f32 and f16 maxima, on the vector path (a whole aligned
    chunk) and on the scalar path (the tail chunk, and a misaligned view)."""
    from flame_amd import engine
    O = _oracle()
    T = engine.chunk_elems(engine.dtype_code(dt))
    numel = 2 * T + 37
    fi = torch.finfo(dt)
    specials = [float("nan"), float("inf"), float("-inf"), fi.smallest_normal / 4, -fi.smallest_normal / 8,
                0.0, -0.0, 65504.0]
    if dt in (torch.float32, torch.float64, torch.bfloat16):
        specials.append(float(torch.tensor(torch.finfo(torch.float32).max).to(dt)) if dt != torch.bfloat16
                        else float(torch.finfo(torch.bfloat16).max))
    g = torch.Generator().manual_seed(9)
    ups, want = [], []
    for c in range(3):
        x = torch.randn(numel, generator=g).to(dt)
        if c < 2:
            for off in ((5, T + 200) if c == 0 else (2 * T + 3,)):      # c = 0: vector chunks; c = 1: the tail
                x[off:off + len(specials)] = torch.tensor(specials, dtype=torch.float64).to(dt)
        ups.append({"x": x})
        want.append(int((~torch.isfinite(x)).sum()))
    assert want[0] == 6 and want[1] == 3 and want[2] == 0
    exact = [_fsum_sq(w.values()) for w in ups]
    for layout in ("tensors", "misaligned", "slab"):
        ws, slab = _layout(ups, layout)
        sumsq, nf = engine.update_stats(ws, DEV)
        _check_stats(f"special/{layout}", sumsq, nf, exact, numel, want)
        assert all(math.isfinite(s) for s in sumsq)
    # keep: the reduction still puts NaN / inf where torch-CPU's ops put them, scaled or not
    out = torch.zeros(numel, dtype=dt, device=DEV)
    engine.reduce_([out], [out], [[w["x"].to(DEV) for w in ups]], [0.25, 0.5, 0.25], scales=[0.5, 1.0, 0.25])
    exp = torch.zeros(numel, dtype=dt)
    O.reduce_tensor(exp, [O.tmp_tensor(w["x"], s) for w, s in zip(ups, [0.5, 1.0, 0.25])], [0.25, 0.5, 0.25])
    S.same_bits("special/scaled", {"x": out}, {"x": exp})


def test_scaled_f16_keeps_every_rounding():
    """fp16: t1 = RN16(RN32(v * scale)), tmp = RN16(RN32(t1 * rate)).  Inputs where ONE rounding of
    the exact product v * scale differs from torch's two (what a fused v_fma_mix* product would
    give), fp16-subnormal results among them; the kernel must match the oracle and torch on all."""
    from flame_amd import engine
    O = _oracle()
    g = torch.Generator().manual_seed(31)
    v = (torch.randn(2_000_000, generator=g) * torch.tensor([1.0, 1e-3, 3e-5]).repeat(666_667)[:2_000_000]).half()
    scale, rate = 0.3713, 0.8125
    s32 = torch.tensor(scale, dtype=torch.float32)
    once = torch.from_numpy((v.double().numpy() * s32.double().item()).astype(np.float16))
    twice = (v.float() * s32).half()
    sel = (once.view(torch.int16) != twice.view(torch.int16)).nonzero().flatten()
    assert sel.numel() > 100, "need double-rounding witnesses"
    vs = v[sel].contiguous()
    out = torch.zeros(vs.numel(), dtype=torch.half, device=DEV)
    engine.reduce_([out], [out], [[vs.to(DEV)]], [rate], scales=[scale])
    exp = torch.zeros(vs.numel(), dtype=torch.half)
    O.reduce_tensor(exp, [O.tmp_tensor(vs, scale)], [rate])
    S.assert_bitwise("f16 scaled product", {"x": out}, {"x": exp})
    S.assert_bitwise("f16 scaled product torch", {"x": out}, {"x": torch.zeros_like(vs) + torch.mul(vs, scale) * rate})


def test_clip_on_the_mixed_dtype_path():
    """Float updates whose dtype is not the aggregate's (bf16 and f16 updates into f32 keys, an f32
    update into a bf16 key) under clip_threshold: each is pre-scaled in ITS dtype
    (engine._prescaled -> tmp_of), then takes the promoted path -- against the oracle's
    tmp_tensor(v, scale) followed by its mixed-dtype reduce_tensor, bitwise.  The int64 update into
    an f32 key (FedOPT's promoted num_batches_tracked) is not scaled."""
    O = _oracle()
    g = torch.Generator().manual_seed(21)
    base = {"a": torch.randn(4099, generator=g), "h": torch.randn(700, generator=g),
            "b": torch.randn(2051, generator=g).bfloat16(), "same": torch.randn(1030, generator=g),
            "nbt": torch.tensor(3.0)}
    ups = []
    for i in range(5):
        s = 0.2 + 0.3 * i
        ups.append({"a": (torch.randn(4099, generator=g) * s).bfloat16(), "h": (torch.randn(700, generator=g) * s).half(),
                    "b": torch.randn(2051, generator=g) * s, "same": torch.randn(1030, generator=g) * s,
                    "nbt": torch.tensor(10 + i)})
    counts = [2, 3, 5, 7, 11]
    clip = 40.0
    opt = _drop_in("fedavg", clip_threshold=clip)
    dev = S.to_dev(base, DEV)
    got = opt.do(dev, _fill(S.SortedCache(), [S.to_dev(u, DEV) for u in ups], counts), total=sum(counts))
    recs = opt.update_stats
    _check_records("mixed", recs, ups, counts, clip)
    assert any(r.scale < 1.0 for r in recs) and any(r.scale == 1.0 for r in recs)
    exp = S.to_cpu(base)
    for u, r, c in zip(ups, recs, counts):
        for k, v in u.items():
            pre = O.tmp_tensor(v, r.scale) if v.is_floating_point() else v
            O.reduce_tensor(exp[k], [pre], [c / sum(counts)])
    S.assert_bitwise("mixed", {k: got[k] for k in base}, exp)


# ---------------------------------------------------------------------------- optimizers
def _drop_in(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


class _MC:
    def __init__(self):
        self.saved = []

    def save(self, mtype, alias, value):
        self.saved.append((mtype, alias, value))


def _model(g, dt, scale, mask=True):
    w = {"w": (torch.randn(4099, generator=g) * scale).to(dt), "b": (torch.randn(3, 70, generator=g) * scale).to(dt),
         "nbt": torch.tensor(int(scale * 10) + 1)}
    if mask:        # FedOPT's d = avg - cur raises on a bool tensor, in the reference as here
        w["mask"] = torch.rand(40, generator=g) > 0.5
    return w


def _fill(cache, ups, counts):
    for i, (u, c) in enumerate(zip(ups, counts)):
        cache[f"e{i:02d}"] = S.TR(u, c)
    return cache


def _float_n(w):
    return sum(v.numel() for v in w.values() if v.is_floating_point())


def _check_records(label, recs, ups, counts, clip):
    """The reported norms / scales against the fsum-derived ones, relative (n + 1) * 2^-53 + 2^-24."""
    assert [r.end for r in recs] == [f"e{i:02d}" for i in range(len(ups))] and [r.count for r in recs] == counts
    for r, u in zip(recs, ups):
        norm = math.sqrt(_fsum_sq(u.values()))
        want = clip / (norm + 1e-6) if norm > clip else 1.0
        tol = (_float_n(u) + 1) * U53 + 2.0 ** -24
        assert abs(r.scale - want) <= tol * want, (label, r, want)
        assert abs(r.norm - norm) <= tol * norm, (label, r, norm)


@pytest.mark.parametrize("sort", ["fedavg", "fedprox", "fedadam"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=IDS[:3])
def test_guarded_optimizers_three_rounds(sort, dt):
    """clip_threshold over 3 rounds: the reported scales (checked against fsum) rebuild the expected
    result with the oracle -- updates pre-scaled with oracle.tmp_tensor, then OracleFedAvg /
    OracleFedOPT.  FedAvg and the FedAvg part of FedOPT bitwise; the FedOPT step under the
    existing contract for fp32 and bitwise for bf16 / fp16.  The int64 0-dim key and the bool
    mask equal the unguarded result."""
    O = _oracle()
    g = torch.Generator().manual_seed(11 + DTYPES.index(dt))
    kw = {"mu": 0.1} if sort == "fedprox" else {}
    clip = 30.0
    adam = sort == "fedadam"
    opt = _drop_in(sort, clip_threshold=clip, **kw)
    plain = _drop_in(sort, **kw)
    ora = O.OracleFedOPT(sort, sqrt_rn=True) if adam else O.OracleFedAvg()
    base = _model(g, dt, 1.0, mask=not adam)
    fkeys = ("w", "b")
    dev_base, dev_plain, ora_base = S.to_dev(base, DEV), S.to_dev(base, DEV), S.to_cpu(base)
    for rnd in range(3):
        n = 9
        ups = [_model(g, dt, 0.1 + 0.1 * i, mask=not adam) for i in range(n)]   # norms from ~6 to ~58: some clipped
        counts = [5 + i for i in range(n)]
        total = sum(counts)
        got = opt.do(dev_base, _fill(S.SortedCache(), [S.to_dev(u, DEV) for u in ups], counts), total=total)
        unguarded = plain.do(dev_plain, _fill(S.SortedCache(), [S.to_dev(u, DEV) for u in ups], counts), total=total)
        recs = opt.update_stats
        _check_records(f"{sort}/r{rnd}", recs, ups, counts, clip)
        assert any(r.scale < 1.0 for r in recs) and any(r.scale == 1.0 for r in recs)
        assert not any(r.skipped or r.nonfinite for r in recs)
        scaled = [{k: (O.tmp_tensor(v, r.scale) if v.is_floating_point() else v.clone()) for k, v in u.items()}
                  for u, r in zip(ups, recs)]
        exp = ora.do(ora_base, _fill(S.SortedCache(), scaled, counts), total=total)
        # the FedAvg part (base_weights, mutated in place): bitwise
        S.assert_bitwise(f"{sort}/r{rnd}/avg", {k: dev_base[k] for k in base}, {k: ora_base[k] for k in base})
        if adam and dt == torch.float32 and rnd > 0:      # the step, each round from identical state
            S.assert_close_fedopt(f"{sort}/r{rnd}", {k: got[k] for k in fkeys}, {k: exp[k] for k in fkeys})
        elif adam and rnd > 0:
            S.assert_bitwise(f"{sort}/r{rnd}/cur", {k: got[k] for k in fkeys}, {k: exp[k] for k in fkeys})
        else:
            S.assert_bitwise(f"{sort}/r{rnd}/cur", {k: got[k] for k in base}, {k: exp[k] for k in base})
        for k in [k for k in base if k not in fkeys]:      # integer / bool keys: as without the guard
            assert torch.equal(dev_base[k].cpu(), dev_plain[k].cpu()), (sort, rnd, k)
            assert torch.equal(got[k].cpu(), unguarded[k].cpu()), (sort, rnd, k)
        if adam:
            # the next round starts from a copy of the new current, as the roles do; the oracle takes
            # the drop-in's state, so every round is compared from identical state
            dev_base = {k: v.clone() for k, v in got.items()}
            dev_plain = {k: v.clone() for k, v in unguarded.items()}
            ora_base = S.to_cpu(got)
            ora.current_weights = S.to_cpu(got)
            if opt.m_t is not None:
                ora.m_t, ora.v_t = S.to_cpu(opt.m_t), S.to_cpu(opt.v_t)


def test_nonfinite_policies_and_metrics():
    """One NaN client out of 9: ``skip`` equals the oracle on the 8 others with the reduced total
    and the model stays finite; ``raise`` raises naming the end and leaves base_weights untouched;
    ``keep`` poisons as the reference does; every client skipped returns None.  The records and
    the three metrics are checked."""
    O = _oracle()
    g = torch.Generator().manual_seed(3)
    base = _model(g, torch.float32, 1.0)
    ups = [_model(g, torch.float32, 0.2) for _ in range(9)]
    ups[4]["w"][77] = float("nan")
    ups[4]["b"][1, 2] = float("inf")
    counts = [4 + i for i in range(9)]
    total = sum(counts)

    def cache():
        return _fill(S.SortedCache(), [S.to_dev(u, DEV) for u in ups], counts)

    # skip (+ a clip that bites on nobody: the plain kernel runs)
    opt = _drop_in("fedavg", nonfinite="skip", clip_threshold=1e6)
    opt.metric_collector = mc = _MC()
    dev = S.to_dev(base, DEV)
    got = opt.do(dev, cache(), total=total)
    keep = [i for i in range(9) if i != 4]
    ora_base = S.to_cpu(base)
    O.OracleFedAvg().do(ora_base, _fill(S.SortedCache(), [S.to_cpu(ups[i]) for i in keep], [counts[i] for i in keep]),
                        total=total - counts[4])
    S.assert_bitwise("skip", {k: got[k] for k in base}, ora_base)
    assert all(bool(torch.isfinite(v).all()) for v in got.values() if v.is_floating_point())
    recs = opt.update_stats
    assert [r.skipped for r in recs] == [i == 4 for i in range(9)] and recs[4].nonfinite == 2
    assert all(r.scale == 1.0 for r in recs) and recs[4].end == "e04" and recs[4].count == counts[4]
    saved = {(m, a): v for m, a, v in mc.saved}
    assert saved[("updates_skipped", "fedavg")] == 1 and saved[("updates_clipped", "fedavg")] == 0
    assert saved[("update_norm_max", "fedavg")] == max(r.norm for r in recs)
    # raise
    opt = _drop_in("fedavg", nonfinite="raise")
    dev = S.to_dev(base, DEV)
    c = cache()
    with pytest.raises(ValueError, match="e04"):
        opt.do(dev, c, total=total)
    S.assert_bitwise("raise leaves base", {k: dev[k] for k in base}, S.to_cpu(base))
    assert len(c) == 0                       # the entries have been popped
    assert [r.nonfinite for r in opt.update_stats] == [2 if i == 4 else 0 for i in range(9)]   # which ends were bad
    assert opt.do(dev, S.SortedCache(), total=0) is None and opt.update_stats == []            # this call's records only
    # keep: the reference's behaviour, NaN where torch-CPU puts it
    opt = _drop_in("fedavg", clip_threshold=1e6)
    dev = S.to_dev(base, DEV)
    got = opt.do(dev, cache(), total=total)
    ora_base = S.to_cpu(base)
    O.OracleFedAvg().do(ora_base, _fill(S.SortedCache(), [S.to_cpu(u) for u in ups], counts), total=total)
    S.same_bits("keep", {k: got[k] for k in base}, ora_base)
    assert opt.update_stats[4].nonfinite == 2 and not opt.update_stats[4].skipped
    # all skipped -> None, base untouched; FedOPT hands back current_weights
    bad = [{k: (torch.full_like(v, float("nan")) if v.is_floating_point() else v.clone()) for k, v in u.items()}
           for u in ups[:2]]
    opt = _drop_in("fedavg", nonfinite="skip")
    dev = S.to_dev(base, DEV)
    assert opt.do(dev, _fill(S.SortedCache(), [S.to_dev(u, DEV) for u in bad], [1, 2]), total=3) is None
    S.assert_bitwise("all skipped", {k: dev[k] for k in base}, S.to_cpu(base))
    assert [r.skipped for r in opt.update_stats] == [True, True]


def test_golden_clipped_fedavg(golden):
    """The reference's own DifferentialPrivacy._apply_clip_norm_torch per client, then its
    FedAvg.do (tests/golden/make_golden_guard.py): the same clients are clipped, the scales agree
    within norm_tol, and the f32 key is within 2 * norm_tol + 2^-22 (rel-L2) of the reference's."""
    import guard_fixture
    fx = golden("fedavg_clipped.npz")
    case = guard_fixture.load(fx)
    opt = _drop_in("fedavg", clip_threshold=case.clip)
    dev = S.to_dev(case.base, DEV)
    got = opt.do(dev, _fill(S.SortedCache(), [S.to_dev(u, DEV) for u in case.updates], case.counts), total=sum(case.counts))
    guard_fixture.check(case, opt.update_stats, {k: v.cpu() for k, v in got.items()})
