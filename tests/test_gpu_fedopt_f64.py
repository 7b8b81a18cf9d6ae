"""GPU: fp64 keys of a FedAdam / FedYogi / FedAdaGrad model through the compiled fp64 kernels
(flame_fedopt_reduce_adapt_f64: one launch per round for all fp64 keys; flame_fedopt_chain_f64:
one launch per deferred eager round), against the reference's statements (fedopt.py:102-129 +
the variant's _delta_v) on the CPU oracle:
  * BITWISE against ``OracleFedOPT(sort, sqrt_rn=True)`` -- every fp64 op one IEEE rounding, the
    root correctly rounded, the scalars the unrounded Python floats -- signed zeros, subnormals,
    overflow and NaNs included (the comparison of tests/test_gpu_elementwise.py: sign bits
    compared, NaN equals NaN);
  * within SURVEY §8(c)'s contract against plain torch-CPU (``OracleFedOPT(sort)``).
Every launch is pinned through the C ABI's launch-branch counters: the fp64 keys take the new
branches and neither the flame_elementwise interpreter nor a separate flame_agg_reduce.
Each round of the syncfl tests starts the oracle from the GPU's state, as
test_fedopt_keys_outside_the_fused_kernel_vs_oracle does.  The base stays on the device."""
import copy
import os
import re

import pytest
import torch

import scenarios as S

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DEV = "cuda:0"
SORTS = ["fedadam", "fedyogi", "fedadagrad"]
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    from oracle import oracle as O
    return O


def _opt(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _chunk(dtype=F64):
    from flame_amd import engine
    return engine.chunk_elems(engine.dtype_code(dtype))


def _client_unroll():
    """kClientUnroll as the library was built: the default of FLAME_T_CLIENT_UNROLL in the source."""
    src = open(os.path.join(ROOT, "flame_amd", "csrc", "fedagg.hip")).read()
    return int(re.search(r"#define FLAME_T_CLIENT_UNROLL (\d+)", src).group(1))


def _counts():
    from flame_amd import _native
    return _native.launch_branch_counts()


def _diff(before, after):
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


def _same(label, got, exp):
    assert set(got.keys()) == set(exp.keys()), (label, list(got.keys()), list(exp.keys()))
    for k in exp:
        g, e = got[k].detach().cpu(), exp[k]
        assert g.dtype == e.dtype and g.shape == e.shape, (label, k, g.dtype, e.dtype, g.shape, e.shape)
        if g.dtype.is_floating_point:
            both_nan = torch.isnan(g) & torch.isnan(e)
            bad = ((g.view(-1) != e.view(-1)) | (torch.signbit(g.view(-1)) != torch.signbit(e.view(-1)))) & ~both_nan.view(-1)
        else:
            bad = g.view(-1) != e.view(-1)
        idx = bad.nonzero().flatten()
        assert idx.numel() == 0, (f"{label}/{k} ({g.dtype}): {idx.numel()} of {g.numel()} differ, first at "
                                  f"{idx[:4].tolist()}: {g.view(-1)[idx[:4]].tolist()} vs {e.view(-1)[idx[:4]].tolist()}")


def _to_dev(w, unaligned=()):
    """The dict on the device; a key in ``unaligned`` as a view one element into its storage
    (8-byte but not 16-byte aligned: the segment is flagged FLAME_SEG_UNALIGNED)."""
    out = {}
    for k, t in w.items():
        if k in unaligned:
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
            buf[1:].copy_(t.reshape(-1))
            out[k] = buf[1:].view(t.shape)
            assert out[k].data_ptr() % 16 == 8 and out[k].is_contiguous()
        else:
            out[k] = t.to(DEV, copy=True)
    return out


def _oracle_round(sort, opt, weights, ups, counts, r, **kw):
    """One syncfl round on a fresh oracle started from the GPU optimizer's state."""
    ora = _oracle().OracleFedOPT(sort, **kw)
    if opt.current_weights is not None:
        ora.current_weights = S.to_cpu(opt.current_weights)
        if opt.m_t is not None:
            ora.m_t, ora.v_t = S.to_cpu(opt.m_t), S.to_cpu(opt.v_t)
    cache, total = S.SortedCache(), sum(counts)
    for i, (u, c) in enumerate(zip(ups, counts)):
        cache[f"r{r}e{i:03d}"] = S.TR({k: t.clone() for k, t in u.items()}, c)
    out = ora.do({k: t.clone() for k, t in weights.items()}, cache, total=total)
    return ora, out


def _check_round(label, opt, got, ora, out):
    _same(f"{label}/current", got, out)
    _same(f"{label}/agg", opt.agg_weights, ora.agg_weights)
    if ora.m_t is not None:
        _same(f"{label}/m", opt.m_t, ora.m_t)
        _same(f"{label}/v", opt.v_t, ora.v_t)
    else:
        assert opt.m_t is None and opt.v_t is None


# ---------------------------------------------------------------- the fused round
@pytest.mark.parametrize("place", ["tensors", "slab"])
@pytest.mark.parametrize("sort", SORTS)
def test_fused_round_vs_oracle(sort, place):
    """Four syncfl rounds of an fp64 model from a fresh optimizer -- the passthrough, the
    zero-state step (FLAME_OPT_STATE_ZERO), two steps with state -- with keys of 1 (0-dim),
    c - 1, c, c + 1 and 3c + 777 elements (c = the fp64 chunk: whole chunks on the vector path,
    ragged tails on the scalar one, more than one workgroup) and one key viewed one element into
    its storage (FLAME_SEG_UNALIGNED); 1, kClientUnroll and kClientUnroll + 1 clients (the
    unrolled client loop, its tail, both), as separate tensors or tiled UpdateSlab slots
    (client_tile_stride).  From round 2 on: exactly one flame_fedopt_reduce_adapt/f64/<variant>
    launch, no flame_elementwise* and no flame_agg_reduce* launch."""
    c, cu = _chunk(), _client_unroll()
    shapes = {"s": (), "a": (c - 1,), "b": (c,), "d": (c + 1,), "e": (3 * c + 777,), "u": (c + 3,)}
    n_clients = [cu + 1, 1, cu, cu + 1]
    g = torch.Generator().manual_seed(101 + SORTS.index(sort))
    weights = {k: torch.randn(s, generator=g, dtype=F64) for k, s in shapes.items()}
    slab = None
    if place == "slab":
        from flame_amd.slab import UpdateSlab
        slab = UpdateSlab({k: torch.empty(s, dtype=F64) for k, s in shapes.items()}, capacity=sum(n_clients), device=DEV)
    opt = _opt(sort)
    name = f"flame_fedopt_reduce_adapt/f64/{sort}"
    for r, n in enumerate(n_clients):
        ups = [{k: torch.randn(s, generator=g, dtype=F64) * 0.1 for k, s in shapes.items()} for _ in range(n)]
        counts = [int(x) for x in torch.randint(1, 50, (n,), generator=g)]
        ora, out = _oracle_round(sort, opt, weights, ups, counts, r, sqrt_rn=True)
        _, out_torch = _oracle_round(sort, opt, weights, ups, counts, r)
        cache = S.SortedCache()
        for i, (u, cnt) in enumerate(zip(ups, counts)):
            w = S.to_dev(u, DEV)
            cache[f"r{r}e{i:03d}"] = S.TR(slab.put(w) if slab is not None else w, cnt)
        base = _to_dev(weights, unaligned=("u",))
        before = _counts()
        got = opt.do(base, cache, total=sum(counts))
        torch.cuda.synchronize()
        hits = _diff(before, _counts())
        label = f"{sort}/{place}/r{r}/n={n}"
        if r >= 1:
            assert hits.get(name) == 1, (label, hits)
            assert sum(v for k, v in hits.items() if k.startswith("flame_fedopt")) == 1, (label, hits)
            assert not any(k.startswith(("flame_elementwise", "flame_agg_reduce")) for k in hits), (label, hits)
        else:
            assert not any(k.startswith("flame_fedopt") for k in hits), (label, hits)
        _check_round(label, opt, got, ora, out)
        S.assert_close_fedopt(f"{label} vs torch-CPU", got, out_torch)
        assert all(t.dtype == F64 for t in got.values())
        weights = S.to_cpu(got)


# ---------------------------------------------------------------- edge values
def _edge_model(c):
    """The fp64 vectors of test_fedopt_int_and_fp64_keys_edge_values (zeros of both signs,
    subnormals, +-1e308, +-1e-300, small normals) and a vector of +-inf and NaN, each as a
    6-element key (scalar path) and at the front of a c-element key (vector path)."""
    f = [[0.0, -0.0, 5e-324, -1e308, 1e-300, 3.5],
         [-0.0, 0.0, 1e-310, 1e308, -1e-300, 2.0],
         [1.0, -2.0, 0.0, -0.0, 7.0, 1e-320]]
    inf, nan = float("inf"), float("nan")
    n = [[inf, -inf, nan, 1.0, -2.0, 0.0],
         [1.0, inf, 2.0, nan, -inf, inf],
         [-inf, 1.0, 0.5, 3.0, inf, -0.0]]
    g = torch.Generator().manual_seed(7)

    def model(i):
        pad = torch.randn(c - 6, generator=g, dtype=F64) * (1.0 if i == 0 else 0.1)
        fv, nv = torch.tensor(f[i], dtype=F64), torch.tensor(n[i], dtype=F64)
        return {"f6": fv, "fc": torch.cat([fv, pad]), "n6": nv, "nc": torch.cat([nv, pad.flip(0)])}
    return model(0), [model(1), model(2)]


@pytest.mark.parametrize("sort", SORTS)
def test_edge_values_bitwise(sort):
    """Signed zeros, subnormals (fp64 denormals are not flushed), overflow to inf, inf and NaN
    operands through the fused fp64 kernel, three rounds, bitwise against the oracle's IEEE
    sequence -- on the vector path and on the scalar path."""
    base, ups = _edge_model(_chunk())
    opt = _opt(sort)
    ora = _oracle().OracleFedOPT(sort, sqrt_rn=True)
    wg, wo = S.to_dev(base, DEV), {k: v.clone() for k, v in base.items()}
    for r in range(3):
        cg, co, total = S.SortedCache(), S.SortedCache(), 0
        for i, u in enumerate(ups):
            total += 3 + i
            cg[f"r{r}e{i}"] = S.TR(S.to_dev(u, DEV), 3 + i)
            co[f"r{r}e{i}"] = S.TR({k: v.clone() for k, v in u.items()}, 3 + i)
        before = _counts()
        wg = opt.do({k: v.clone() for k, v in wg.items()}, cg, total=total)
        torch.cuda.synchronize()
        hits = _diff(before, _counts())
        wo = ora.do(copy.deepcopy(wo), co, total=total)
        if r >= 1:
            assert hits == {f"flame_fedopt_reduce_adapt/f64/{sort}": 1}, hits
        _check_round(f"{sort}/r{r}", opt, wg, ora, wo)


# ---------------------------------------------------------------- the eager caller's aliased step
@pytest.mark.parametrize("sort", SORTS)
def test_eager_aliased_step_fused_f64(sort):
    """test_fedopt_eager_aliased_step_fused in fp64: the same base dict goes to every do(), so
    after the round-1 passthrough current_weights IS base; that step is one fused fp64 launch
    with FLAME_SEG_CUR_IS_AVG (d = avg - avg), bitwise against the oracle, as are the steps after."""
    c = _chunk()
    g = torch.Generator().manual_seed(17)
    shapes = {"a": (c + 5,), "b": (37,)}
    base0 = {k: torch.randn(s, generator=g, dtype=F64) for k, s in shapes.items()}
    ups = [{k: torch.randn(s, generator=g, dtype=F64) * 1e-2 for k, s in shapes.items()} for _ in range(4)]
    counts = [7, 3, 9, 2]
    opt = _opt(sort)
    ora = _oracle().OracleFedOPT(sort, sqrt_rn=True)
    bw = S.to_dev(base0, DEV)
    ob = {k: v.clone() for k, v in base0.items()}
    running = 0
    for i, u in enumerate(ups):
        running += counts[i]
        cg, co = S.SortedCache(), S.SortedCache()
        cg[f"e{i}"] = S.TR(S.to_dev(u, DEV), counts[i])
        co[f"e{i}"] = S.TR({k: v.clone() for k, v in u.items()}, counts[i])
        before = _counts()
        got = opt.do(bw, cg, total=running, num_trainers=4)
        torch.cuda.synchronize()
        hits = _diff(before, _counts())
        exp = ora.do(ob, co, total=running)
        if i >= 1:
            assert hits == {f"flame_fedopt_reduce_adapt/f64/{sort}": 1}, (i, hits)
        if i == 1:          # d = avg - avg = 0: the step leaves current at the average
            _same(f"eager/{sort}/step1/cur==avg", got, ob)
        _same(f"eager/{sort}/step{i}/cur", got, exp)
        _same(f"eager/{sort}/step{i}/avg", bw, ob)
        if ora.m_t is not None:
            _same(f"eager/{sort}/step{i}/m", opt.m_t, ora.m_t)
            _same(f"eager/{sort}/step{i}/v", opt.v_t, ora.v_t)


# ---------------------------------------------------------------- the deferred eager chain
def _chain_models(model):
    c64, c32 = _chunk(F64), _chunk(torch.float32)
    keys = [("a", F64, c64), ("b", F64, c64 + 5)]
    if model == "f32+f64":
        keys = [("p", torch.float32, c32), *keys, ("q", torch.float32, c32 + 5)]
    return keys


def _eager_rounds(opt, w0, rounds, to_dev, on_round=None):
    """The eager role's calls (one do() per arrival into the round's base, running total; an
    arrival of ``None`` has an empty cache); per round (base, current, m_t, v_t) on the CPU."""
    weights, res = to_dev(w0), []
    for r, calls in enumerate(rounds):
        base = {k: v.clone() for k, v in dict(weights).items()}
        total, out = 0, None
        before = _counts()
        for i, call in enumerate(calls):
            cache = S.SortedCache()
            if call is not None:
                u, cnt = call
                total += cnt
                cache[f"r{r}e{i:03d}"] = S.TR(to_dev(u), cnt)
            out = opt.do(base, cache, total=total, num_trainers=len(calls))
        weights = out
        cur = S.to_cpu(dict(out))             # the read runs the deferred queue
        if on_round is not None:
            torch.cuda.synchronize()
            on_round(r, _diff(before, _counts()))
        res.append((S.to_cpu(base), cur, S.to_cpu(opt.m_t), S.to_cpu(opt.v_t)))
    return res


@pytest.mark.parametrize("model", ["f64", "f32+f64"])
@pytest.mark.parametrize("sort", SORTS)
def test_deferred_chain_f64(sort, model):
    """FedOPT(defer=True) on an fp64 and on a mixed f32 + f64 model (keys of c and c + 5
    elements): two eager rounds of 5 arrivals, the second with an arrival that has nothing to
    aggregate in its middle.  Per round exactly one flame_fedopt_chain/f64/<variant> launch (and
    one f32 chain launch for the mixed model); base, current, m_t and v_t bitwise equal to the
    oracle's per-call do() and to a non-deferred GPU optimizer fed the same arrivals."""
    keys = _chain_models(model)
    g = torch.Generator().manual_seed(211 + SORTS.index(sort))
    w0 = {k: torch.randn(n, generator=g, dtype=F64).to(dt) for k, dt, n in keys}
    rounds = []
    for r in range(2):
        calls = [({k: (torch.randn(n, generator=g, dtype=F64) * 1e-2).to(dt) for k, dt, n in keys},
                  int(torch.randint(1, 500, (1,), generator=g))) for _ in range(5)]
        if r == 1:
            calls.insert(3, None)
        rounds.append(calls)
    want = {f"flame_fedopt_chain/f64/{sort}": 1}
    if model == "f32+f64":
        want[f"flame_fedopt_chain/f32/{sort}"] = 1
    seen = []

    def on_round(r, hits):
        seen.append(hits)
        assert {k: v for k, v in hits.items() if k.startswith("flame_fedopt")} == want, (r, hits)
        assert not any(k.startswith("flame_elementwise") for k in hits), (r, hits)
    got = _eager_rounds(_opt(sort, defer=True), w0, rounds, lambda w: S.to_dev(w, DEV), on_round)
    assert len(seen) == 2
    ref = _eager_rounds(_opt(sort), w0, rounds, lambda w: S.to_dev(w, DEV))
    ora = _eager_rounds(_oracle().OracleFedOPT(sort, sqrt_rn=True), w0, rounds,
                        lambda w: {k: v.clone() for k, v in w.items()})
    for r in range(2):
        for lbl, x, y, z in zip(("base", "current", "m_t", "v_t"), got[r], ref[r], ora[r]):
            _same(f"{sort}/{model}/r{r}/{lbl} vs per-call launches", x, y)
            _same(f"{sort}/{model}/r{r}/{lbl} vs oracle", x, z)


# ---------------------------------------------------------------- a mixed model through do()
@pytest.mark.parametrize("sort", SORTS)
def test_mixed_model_through_do(sort):
    """f32, bf16 and f64 keys beside an int64 0-dim num_batches_tracked: the float keys take the
    fused kernel of their dtype (f64 the new one), the int64 key still runs as a flame_elementwise
    program; every key bitwise against the oracle, each round from the GPU's state."""
    c = _chunk()
    spec = {"w": (torch.float32, (300,)), "h": (torch.bfloat16, (64,)), "d": (F64, (c + 9,)),
            "bn.num_batches_tracked": (torch.int64, ())}
    g = torch.Generator().manual_seed(311 + SORTS.index(sort))

    def draw(scale, bump):
        return {k: ((torch.randn(s, generator=g, dtype=F64) * scale).to(dt) if dt.is_floating_point
                    else torch.randint(0, 1000, s, generator=g) + bump) for k, (dt, s) in spec.items()}
    weights = draw(1.0, 0)
    opt = _opt(sort)
    for r in range(3):
        ups = [draw(0.1, 10 * r + i) for i in range(3)]
        counts = [int(x) for x in torch.randint(1, 50, (3,), generator=g)]
        ora, out = _oracle_round(sort, opt, weights, ups, counts, r, sqrt_rn=True)
        cache = S.SortedCache()
        for i, (u, cnt) in enumerate(zip(ups, counts)):
            cache[f"r{r}e{i:03d}"] = S.TR(S.to_dev(u, DEV), cnt)
        before = _counts()
        got = opt.do(S.to_dev(weights, DEV), cache, total=sum(counts))
        torch.cuda.synchronize()
        hits = _diff(before, _counts())
        if r >= 1:
            assert hits.get(f"flame_fedopt_reduce_adapt/f64/{sort}") == 1, hits
            assert hits.get("flame_elementwise") == 1 and "flame_elementwise_segments" not in hits, hits
            fused = {k.split("/")[1]: v for k, v in hits.items() if k.startswith("flame_fedopt")}
            assert fused == {"f32": 1, "bf16": 1, "f64": 1}, hits
        _check_round(f"{sort}/mixed/r{r}", opt, got, ora, out)
        assert got["d"].dtype == F64
        weights = S.to_cpu(got)
        # the trainers' BatchNorm keeps counting in int64 whatever the step returned (fp32)
        weights["bn.num_batches_tracked"] = torch.tensor(100 * (r + 1), dtype=torch.int64)
