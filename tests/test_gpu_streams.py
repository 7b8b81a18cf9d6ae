"""GPU: every device path under a non-default current stream whose inputs become valid late.

The rest of the suite pins the arithmetic on torch's default stream with inputs that are complete
before the call.  These tests pin WHEN the library's work runs: tests/stream_case.py fills every
buffer the library will read with poison, enters ``torch.cuda.stream(s)``, enqueues a delay and only
behind it the copies that write the true values, then calls the library.  A launch, copy or readback
that is not ordered behind ``s`` sees poison and the bitwise comparison with the CPU oracle
(oracle/oracle.py; ``trim``: tests/trimmed_ref.py; ``krum``: tests/krum_ref.py) fails.  Each case
also runs with everything ready on the default stream and must give the same bits (secondary).

Asynchronous entry points carry ``Late.call``'s "the delay is still running" assertion.  Those that
synchronise by contract name the documented synchronisation instead (``sync=...``): the guard's and
krum's one readback (engine.update_stats / update_gram), a host-resident target's write-back, and
egress.

The model: fp32 keys of 0, 1, 1023, 1024 and 4099 elements (a chunk is 1,024 fp32 elements), a bf16
key of 3 * 2048 + 5 elements shaped (-1, 1), an fp64 key of 1025 elements, an int64 0-dim key.
"""
import functools
import math
from collections import OrderedDict

import pytest
import torch

import scenarios as S
import stream_case as SC

pytestmark = [pytest.mark.gpu]
oracle = pytest.mark.oracle

DEV = SC.DEV
KEYS = [("z", torch.float32, (0,)), ("one", torch.float32, (1,)), ("a", torch.float32, (1023,)),
        ("b", torch.float32, (1024,)), ("w", torch.float32, (4099,)), ("h", torch.bfloat16, (3 * 2048 + 5, 1)),
        ("d", torch.float64, (1025,)), ("nbt", torch.int64, ())]
FLOAT_KEYS = tuple(k for k, dt, _ in KEYS if dt.is_floating_point)
N = 7
COUNTS = [3, 1, 4, 1, 5, 9, 2]
TOTAL = sum(COUNTS)
ROUNDS = 3


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()
    torch.empty(1, device=DEV)


@pytest.fixture(scope="module")
def delay():
    d = SC.Delay()
    print(f"stream_case: delay {d.ms} ms = {d.ops} adds over {SC.DELAY_BYTES >> 20} MiB ({d.ms_per_op:.4f} ms each)")
    yield d
    d.free()


def _oracle():
    from oracle import oracle as O
    return O


def make_amd(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _tensor(g, dt, shape, scale, ival):
    if dt == torch.float64:
        return torch.randn(shape, generator=g, dtype=torch.float64) * scale
    if dt.is_floating_point:
        return (torch.randn(shape, generator=g) * scale).to(dt)
    return torch.full(shape, ival, dtype=dt)


@functools.lru_cache(maxsize=None)
def _data(n=N, keys=None, rounds=ROUNDS):
    """(base, ups[round][i]) on the CPU, built once, never modified."""
    g = torch.Generator().manual_seed(7100 + n)
    spec = [s for s in KEYS if keys is None or s[0] in keys]
    base = OrderedDict((k, _tensor(g, dt, sh, 1.0, 7)) for k, dt, sh in spec)
    ups = [[OrderedDict((k, _tensor(g, dt, sh, 1e-2, 100 + 37 * i)) for k, dt, sh in spec) for i in range(n)]
           for _ in range(rounds)]
    return base, ups


def _clone(w):
    return OrderedDict((k, v.clone()) for k, v in w.items())


def _fill(ups, counts, ends=None, versions=None, cache=None):
    cache = S.SortedCache() if cache is None else cache
    for i, (u, c) in enumerate(zip(ups, counts)):
        cache[ends[i] if ends is not None else f"e{i:02d}"] = S.TR(u, c, versions[i] if versions is not None else 0)
    return cache


def _poisoned_cache(placement):
    """A DeviceUpdateCache; a slab one gets its slab now, every slot holding poison (a new slab is
    torch.empty: the allocator may hand it the block of an earlier test's slab, true values and all)."""
    from flame_amd.ingest import DeviceUpdateCache
    from flame_amd.slab import UpdateSlab
    cache = DeviceUpdateCache(device=DEV, placement=placement, capacity=N)
    if placement == "slab":
        cache.slab = UpdateSlab(_data()[1][0][0], N, DEV)
        for st in cache.slab.storage.values():
            st.fill_(SC.POISON)
    return cache


def _both(label, case, delay):
    """``case(L)`` with everything ready on the default stream, then late on a stream of its own:
    each compares with the reference itself; the two must also agree bit for bit."""
    ready = case(SC.Late(delay, ready=True))
    late = case(SC.Late(delay))
    SC.assert_same(label, ready, late)


# ------------------------------------------------------------------ 1. the plain reduction
SOURCES = ["tensors", "slab-host", "slab-dev", "hbm-host", "hbm-dev", "host"]


def _fedavg_case(src, label, exp, recorder=False):
    from flame_amd import metrics
    base0, ups = _data()

    def case(L):
        base = L.weights(base0)
        cache = _poisoned_cache(src.split("-")[0]) if src != "tensors" else None
        if src == "tensors" or src.endswith("-dev"):
            srcs = [L.weights(u) for u in ups[0]]
        elif src == "host":
            srcs = [L.weights(u, "pinned") for u in ups[0]]
        else:
            srcs = [_clone(u) for u in ups[0]]          # pageable, as a channel delivers them
        rec = metrics.KernelRecorder() if recorder else None
        with L.stream():
            L.start()
            if rec is not None:
                rec.__enter__()
            try:
                if src == "tensors":
                    cache = _fill([OrderedDict(u) for u in srcs], COUNTS)
                else:
                    with L.call(f"insert/{label}"):
                        if src == "slab-dev":       # the inserts below run late on the side stream (Delay.ballast)
                            cache["ballast"] = S.TR(L.delay.ballast(), 0)
                        _fill([OrderedDict(u) for u in srcs], COUNTS, cache=cache)
                    if src == "slab-dev":
                        assert len(cache.slab._free) == 0, "the ballast took no slot (other keys: the hbm route)"
                        cache.pop("ballast")
                    if src.endswith("-dev"):
                        # a device source may be dropped (not rewritten) once the insert has returned
                        L.reuse(*srcs)
                with L.call(f"do/{label}"):
                    out = make_amd("fedavg").do(base, cache, total=TOTAL)
            finally:
                if rec is not None:
                    rec.__exit__(None, None, None)
            assert out is base and len(cache) == 0
            if src == "tensors":
                L.reuse(*srcs)
            got = L.snap(out)
        L.finish()
        S.assert_bitwise(label, got, exp)
        if rec is not None:
            assert len(rec) >= 3 and rec.ready(), label      # one launch per dtype group at least
            for name, e0, e1, _ in rec:
                ms = e0.elapsed_time(e1)
                assert math.isfinite(ms) and ms >= 0.0, (label, name, ms)
        return {"out": got}
    return case


def _fedavg_expected():
    base0, ups = _data()
    return _oracle().OracleFedAvg().do(_clone(base0), _fill([_clone(u) for u in ups[0]], COUNTS), total=TOTAL)


@oracle
@pytest.mark.parametrize("argmeta", [True, False], ids=["argmeta", "table"])
@pytest.mark.parametrize("src", SOURCES)
def test_fedavg_late_updates(src, argmeta, delay, monkeypatch):
    """FedAvg.do over late device tensors, a DeviceUpdateCache of every placement (host sources, and
    device sources revealed late before ``cache[key] = ...``), and pinned zero-copy updates; with the
    metadata in the kernel arguments and as a device table (the only path through _Staging.upload)."""
    from flame_amd import engine
    if not argmeta:
        monkeypatch.setattr(engine, "ARGMETA", False)
    label = f"fedavg/{src}/{'argmeta' if argmeta else 'table'}"
    _both(label, _fedavg_case(src, label, _fedavg_expected()), delay)


@oracle
def test_fedavg_recorder_on(delay):
    """Case 1 (slab, device sources) inside an active KernelRecorder: every event pair gives a finite,
    non-negative elapsed_time after the stream is synchronised, and the bits are still right."""
    _both("fedavg/recorder", _fedavg_case("slab-dev", "fedavg/recorder", _fedavg_expected(), recorder=True), delay)


@oracle
@pytest.mark.parametrize("argmeta", [True, False], ids=["argmeta", "table"])
def test_reduce_init_first(argmeta, delay, monkeypatch):
    """engine.reduce_ with FLAME_AGG_INIT_FIRST (the first client initialises the output: no base is
    read) and without, over the non-empty keys."""
    from flame_amd import engine
    O = _oracle()
    if not argmeta:
        monkeypatch.setattr(engine, "ARGMETA", False)
    base0, ups = _data()
    keys = [k for k in FLOAT_KEYS if base0[k].numel()]
    rates = [c / TOTAL for c in COUNTS]
    exp = {}
    for init_first in (False, True):
        e = OrderedDict()
        for k in keys:
            acc = base0[k].clone()
            cl = [u[k] for u in ups[0]]
            if init_first:      # (the oracle's init_first keeps the call's last client: split the call)
                O.reduce_tensor(acc, cl[:1], rates[:1], init_first=True)
                O.reduce_tensor(acc, cl[1:], rates[1:])
            else:
                O.reduce_tensor(acc, cl, rates)
            e[k] = acc
        exp[init_first] = e

    def case(L):
        res = {}
        outs = {f: L.weights(OrderedDict((k, base0[k]) for k in keys), group=0) for f in (False, True)}
        srcs = [L.weights(OrderedDict((k, u[k]) for k in keys)) for u in ups[0]]
        with L.stream():
            L.start()
            for init_first in (False, True):
                o = [outs[init_first][k] for k in keys]
                with L.call(f"reduce_/init_first={init_first}"):
                    engine.reduce_(o, None if init_first else o, [[u[k] for u in srcs] for k in keys], rates,
                                   init_first=init_first)
                res[f"init_first={init_first}"] = L.snap(outs[init_first])
            L.reuse(*srcs)
        L.finish()
        for init_first in (False, True):
            S.assert_bitwise(f"reduce_/init_first={init_first}", res[f"init_first={init_first}"], exp[init_first])
        return res
    _both("reduce_", case, delay)


# ------------------------------------------------------------------ 2. slot reuse
@oracle
@pytest.mark.parametrize("source", ["host", "dev"])
def test_slab_slots_reused_across_rounds(source, delay):
    """Three rounds over a slab of exactly one round's capacity: rounds 2 and 3 write into the slots
    the previous do() released (slab._release's event on the launch stream, slab.write's wait on
    it), all under ``s`` with a delay in front of every round's inserts."""
    O = _oracle()
    base0, ups = _data()
    exps, w = [], _clone(base0)
    for r in range(ROUNDS):
        w = O.OracleFedAvg().do(_clone(w), _fill([_clone(u) for u in ups[r]], COUNTS), total=TOTAL)
        exps.append(_clone(w))

    def case(L):
        base = L.weights(base0)
        srcs = [[L.weights(u, group=r) if source == "dev" else _clone(u) for u in ups[r]] for r in range(ROUNDS)]
        cache = _poisoned_cache("slab")
        opt = make_amd("fedavg")
        res = {}
        with L.stream():
            for r in range(ROUNDS):
                L.start(group=r)
                with L.call(f"reuse/{source}/insert r{r}"):
                    _fill([OrderedDict(u) for u in srcs[r]], COUNTS, cache=cache)
                assert cache.slab is not None and not cache.slab._free, "every slot taken: the next round reuses them"
                with L.call(f"reuse/{source}/do r{r}"):
                    out = opt.do(base, cache, total=TOTAL)
                assert len(cache.slab._free) == N
                res[f"r{r}"] = L.snap(out)
        L.finish()
        for r in range(ROUNDS):
            S.assert_bitwise(f"reuse/{source}/r{r}", res[f"r{r}"], exps[r])
        return res
    _both(f"reuse/{source}", case, delay)


# ------------------------------------------------------------------ 3. FedOPT
FEDOPT_ROWS = {"fedadam": ("fedadam", {}), "fedyogi": ("fedyogi", {}), "fedadagrad": ("fedadagrad", {}),
               "fedadam-defer": ("fedadam", {"defer": True})}


def _fedopt_expected(sort):
    """Per round: the oracle's state BEFORE it (current, m, v) and its results (avg, current, m, v)."""
    O = _oracle()
    base0, ups = _data()
    ora = O.OracleFedOPT(sort, sqrt_rn=True)
    cur = _clone(base0)
    rounds = []
    for r in range(ROUNDS):
        before = {"cur": _clone(cur), "m": _clone(ora.m_t) if ora.m_t else None, "v": _clone(ora.v_t) if ora.v_t else None}
        exp = ora.do(_clone(cur), _fill([_clone(u) for u in ups[r]], COUNTS), total=TOTAL)
        rounds.append((before, {"avg": _clone(ora.agg_weights), "cur": _clone(exp),
                                "m": _clone(ora.m_t) if ora.m_t else None, "v": _clone(ora.v_t) if ora.v_t else None}))
        cur = _clone(exp)
    return rounds


def _fedopt_case(row, label, streams=None):
    """Round 0 is the passthrough, rounds 1 and 2 the fused reduce + adapt.  Before rounds 1 and 2 the
    base, ``current_weights`` and (once they exist) ``m_t`` / ``v_t`` are replaced by late buffers
    holding the oracle's state, which the previous round was compared with."""
    sort, kw = FEDOPT_ROWS[row]
    _, ups = _data()
    rounds = _fedopt_expected(sort)

    def case(L):
        opt = make_amd(sort, **kw)
        bases = [L.weights(rounds[r][0]["cur"], group=r) for r in range(ROUNDS)]
        curs = [None] + [L.weights(rounds[r][0]["cur"], group=r) for r in range(1, ROUNDS)]
        ms = [L.weights(rounds[r][0]["m"], group=r) if rounds[r][0]["m"] else None for r in range(ROUNDS)]
        vs = [L.weights(rounds[r][0]["v"], group=r) if rounds[r][0]["v"] else None for r in range(ROUNDS)]
        srcs = [[L.weights(u, group=r) for u in ups[r]] for r in range(ROUNDS)]
        res = {}
        for r in range(ROUNDS):
            with _round_stream(L, streams, r):
                if curs[r] is not None:
                    opt.current_weights = curs[r]
                if ms[r] is not None:
                    opt.m_t, opt.v_t = dict(ms[r]), dict(vs[r])
                L.start(group=r)
                with L.call(f"{label}/r{r}"):
                    got = opt.do(bases[r], _fill([OrderedDict(u) for u in srcs[r]], COUNTS), total=TOTAL)
                    got = OrderedDict((k, got[k]) for k in got)       # (a DeferredCurrent runs its queue here)
                L.reuse(*srcs[r])
                res[f"r{r}/avg"], res[f"r{r}/cur"] = L.snap(bases[r]), L.snap(got)
                if opt.m_t is not None:
                    res[f"r{r}/m"], res[f"r{r}/v"] = L.snap(opt.m_t), L.snap(opt.v_t)
        _finish(L, streams)
        for r in range(ROUNDS):
            exp = rounds[r][1]
            S.same_bits(f"{label}/r{r}/avg", res[f"r{r}/avg"], exp["avg"])
            S.same_bits(f"{label}/r{r}/cur", res[f"r{r}/cur"], exp["cur"])
            assert (f"r{r}/m" in res) == (exp["m"] is not None), label
            if exp["m"] is not None:
                S.same_bits(f"{label}/r{r}/m", res[f"r{r}/m"], exp["m"])
                S.same_bits(f"{label}/r{r}/v", res[f"r{r}/v"], exp["v"])
        return res
    return case


@oracle
@pytest.mark.parametrize("row", list(FEDOPT_ROWS))
def test_fedopt_late_state(row, delay):
    _both(row, _fedopt_case(row, row), delay)


# ------------------------------------------------------------------ 4. FedBuff and the hierarchies
@oracle
@pytest.mark.parametrize("with_delta", [False, True], ids=["scale_add", "with_delta"])
def test_fedbuff_scale_add(with_delta, delay):
    """do(None, ...) over late arrivals (the first one initialises the aggregate), then the fused
    scale_add into a late model, with and without the upload delta."""
    O = _oracle()
    base0, ups = _data(N, FLOAT_KEYS)
    versions = [10 - (i % 4) for i in range(N)]
    ora = O.OracleFedBuff()
    oagg = ora.do(None, _fill([_clone(u) for u in ups[0]], COUNTS, versions=versions), total=TOTAL, version=10)
    ow = _clone(base0)
    ora.scale_add_agg_weights(ow, oagg, N)
    odelta = OrderedDict((k, ow[k] - base0[k]) for k in ow)
    label = f"fedbuff/delta={with_delta}"

    def case(L):
        opt = make_amd("fedbuff")
        base = L.weights(base0)
        srcs = [L.weights(u) for u in ups[0]]
        with L.stream():
            L.start()
            with L.call(label):
                agg = opt.do(None, _fill([OrderedDict(u) for u in srcs], COUNTS, versions=versions), total=TOTAL, version=10)
                if with_delta:
                    out, delta = opt.scale_add_agg_weights_with_delta(base, agg, N)
                else:
                    out, delta = opt.scale_add_agg_weights(base, agg, N), None
            L.reuse(*srcs)
            res = {"out": L.snap(out), "agg": L.snap(OrderedDict((k, agg[k]) for k in agg))}
            if delta is not None:
                res["delta"] = L.snap(delta)
        L.finish()
        assert out is base
        S.assert_bitwise(f"{label}/out", res["out"], ow)
        S.assert_bitwise(f"{label}/agg", res["agg"], oagg)
        if with_delta:
            S.assert_bitwise(f"{label}/delta", res["delta"], odelta)
        return res
    _both(label, case, delay)


@oracle
def test_fedbuff_hierarchy_round(delay):
    """The one-pass hierarchy (flame_hier_fedbuff): 3 middles x 3 arrivals; the arrivals, the middles'
    weights, the top's running aggregate and the top's model are all revealed late."""
    from flame_amd.optimizer.fedbuff import hierarchy_round
    O = _oracle()
    M, A, rnd = 3, 3, 12
    base0, ups = _data(M * A, FLOAT_KEYS)
    g = torch.Generator().manual_seed(99)
    mid0 = [OrderedDict((k, v + 0.25 * m) for k, v in base0.items()) for m in range(M)]
    top_prev = OrderedDict((k, _tensor(g, v.dtype, v.shape, 1e-3, 0)) for k, v in base0.items())
    top_w0 = OrderedDict((k, v * 0.5) for k, v in base0.items())
    vers = [[rnd - (m + t) % 3 for t in range(A)] for m in range(M)]
    mid_ver = [rnd - m % 2 for m in range(M)]
    oaggs = []
    for m in range(M):
        mo, ao = O.OracleFedBuff(), None
        for t in range(A):
            c = S.SortedCache()
            c["a"] = S.TR(_clone(ups[0][m * A + t]), 1, vers[m][t])
            ao = mo.do(ao, c, total=1, version=rnd)
        oaggs.append(ao)
    omids, otw = [_clone(w) for w in mid0], _clone(top_w0)
    oagg, odeltas = S.oracle_hierarchy_round([(omids[m], oaggs[m], A, mid_ver[m]) for m in range(M)], _clone(top_prev),
                                             version=rnd, top_weights=otw, top_goal=M, with_delta=True)

    def case(L):
        srcs = [L.weights(u) for u in ups[0]]
        mids = [L.weights(w) for w in mid0]
        ta, tw = L.weights(top_prev), L.weights(top_w0)
        with L.stream():
            L.start()
            with L.call("hier_fedbuff"):
                aggs = []
                for m in range(M):
                    opt, agg = make_amd("fedbuff"), None
                    for t in range(A):
                        c = S.SortedCache()
                        c["a"] = S.TR(OrderedDict(srcs[m * A + t]), 1, vers[m][t])
                        agg = opt.do(agg, c, total=1, version=rnd)
                    aggs.append(agg)
                agg, deltas = hierarchy_round([(mids[m], aggs[m], A, mid_ver[m]) for m in range(M)], ta, version=rnd,
                                              top_weights=tw, top_goal=M, with_delta=True)
            del aggs
            L.reuse(*srcs)
            res = {"agg": L.snap(OrderedDict((k, agg[k]) for k in agg)), "top": L.snap(tw)}
            for m in range(M):
                res[f"mid{m}"], res[f"delta{m}"] = L.snap(mids[m]), L.snap(deltas[m])
        L.finish()
        S.assert_bitwise("hier/agg", res["agg"], oagg)
        S.assert_bitwise("hier/top", res["top"], otw)
        for m in range(M):
            S.assert_bitwise(f"hier/mid{m}", res[f"mid{m}"], omids[m])
            S.assert_bitwise(f"hier/delta{m}", res[f"delta{m}"], odeltas[m])
        return res
    _both("hier_fedbuff", case, delay)


@oracle
def test_sync_hierarchy_round(delay):
    """The synchronous hierarchy: 2 middles x 3 arrivals; arrivals, middles and top revealed late."""
    from flame_amd.optimizer.sync_hierarchy import sync_hierarchy_round
    _oracle()
    base0, ups = _data(6)
    mid_counts = [[1, 2, 3], [4, 5, 6]]
    otop = OrderedDict((k, v * 0.5 if v.is_floating_point() else v.clone()) for k, v in base0.items())
    top0 = _clone(otop)
    omids = [_clone(base0) for _ in range(2)]
    ospecs = [(omids[j], _fill([_clone(u) for u in ups[0][3 * j:3 * j + 3]], mid_counts[j]), sum(mid_counts[j]))
              for j in range(2)]
    _, odeltas = S.oracle_sync_hierarchy_round(ospecs, otop, with_delta=True)

    def case(L):
        srcs = [L.weights(u) for u in ups[0]]
        mids, top = [L.weights(base0) for _ in range(2)], L.weights(top0)
        with L.stream():
            L.start()
            specs = [(mids[j], _fill([OrderedDict(u) for u in srcs[3 * j:3 * j + 3]], mid_counts[j]), sum(mid_counts[j]))
                     for j in range(2)]
            with L.call("sync_hierarchy"):
                out, deltas = sync_hierarchy_round(specs, top, with_delta=True)
            del specs
            L.reuse(*srcs)
            res = {"top": L.snap(top)}
            for j in range(2):
                res[f"mid{j}"], res[f"delta{j}"] = L.snap(mids[j]), L.snap(deltas[j])
        L.finish()
        assert out is top
        S.assert_bitwise("sync/top", res["top"], otop)
        for j in range(2):
            S.assert_bitwise(f"sync/mid{j}", res[f"mid{j}"], omids[j])
            S.assert_bitwise(f"sync/delta{j}", res[f"delta{j}"], odeltas[j])
        return res
    _both("sync_hierarchy", case, delay)


# ------------------------------------------------------------------ 5. FedDyn and SCAFFOLD
DYN_ENDS = [f"t{i}" for i in range(N + 1)]
# t7 joins in round 1 while t0 is away; t0 returns in round 2 (its history kept meanwhile)
DYN_ROUNDS = [DYN_ENDS[0:N], DYN_ENDS[1:N + 1], DYN_ENDS[0:N]]


def _feddyn_expected():
    O = _oracle()
    base0, ups = _data()
    ora = O.OracleFedDyn(alpha=0.01)
    w = _clone(base0)
    rounds = []
    for r, ends in enumerate(DYN_ROUNDS):
        ora.save_state(S._PRE, active_ends=DYN_ENDS)
        before = {"w": _clone(w), "cld": _clone(ora.cld_model) if r else None,
                  "hist": {e: (_clone(h) if h is not None else None) for e, h in ora.local_param_dict.items()}}
        exp = ora.do(_clone(w), _fill([_clone(u) for u in ups[r]], COUNTS, ends=ends), total=TOTAL)
        rounds.append((before, {"avg": _clone(exp), "cld": _clone(ora.cld_model),
                                "hist": {e: (_clone(h) if h is not None else None)
                                         for e, h in ora.local_param_dict.items()}}))
        w = _clone(ora.cld_model)
    return rounds


def _feddyn_case(history, label, streams=None):
    """Before rounds 1 and 2 ``cld_model`` and every history are replaced by late buffers holding the
    oracle's state (ping-pong: FedDyn._pp_adopt writes them back into the slab stores with
    ``write_key`` on the current stream)."""
    _, ups = _data()
    rounds = _feddyn_expected()

    def case(L):
        opt = make_amd("feddyn", alpha=0.01, history=history)
        bases = [L.weights(rounds[r][0]["w"], group=r) for r in range(ROUNDS)]
        clds = [L.weights(rounds[r][0]["cld"], group=r) if r else None for r in range(ROUNDS)]
        hists = [{e: L.weights(h, group=r) for e, h in rounds[r][0]["hist"].items() if h is not None} if r else {}
                 for r in range(ROUNDS)]
        srcs = [[L.weights(u, group=r) for u in ups[r]] for r in range(ROUNDS)]
        res = {}
        for r, ends in enumerate(DYN_ROUNDS):
            with _round_stream(L, streams, r):
                opt.save_state(S._PRE, active_ends=DYN_ENDS)
                if r:
                    opt.cld_model = dict(clds[r])
                    for e, h in hists[r].items():
                        assert opt.local_param_dict[e] is not None, (label, r, e)
                        opt.local_param_dict[e] = dict(h)
                L.start(group=r)
                with L.call(f"{label}/r{r}"):
                    out = opt.do(bases[r], _fill([OrderedDict(u) for u in srcs[r]], COUNTS, ends=ends), total=TOTAL)
                L.reuse(*srcs[r])
                res[f"r{r}/avg"], res[f"r{r}/cld"] = L.snap(out), L.snap(opt.cld_model)
                assert [e for e, h in opt.local_param_dict.items() if h is not None] == \
                    [e for e, h in rounds[r][1]["hist"].items() if h is not None], label
                for e, h in opt.local_param_dict.items():
                    if h is not None:
                        res[f"r{r}/hist/{e}"] = L.snap(OrderedDict((k, h[k]) for k in rounds[r][1]["hist"][e]))
        _finish(L, streams)
        for r in range(ROUNDS):
            exp = rounds[r][1]
            S.assert_bitwise(f"{label}/r{r}/avg", res[f"r{r}/avg"], exp["avg"])
            S.assert_bitwise(f"{label}/r{r}/cld", res[f"r{r}/cld"], exp["cld"])
            for e, h in exp["hist"].items():
                if h is not None:
                    S.assert_bitwise(f"{label}/r{r}/hist/{e}", res[f"r{r}/hist/{e}"], h)
        return res
    return case


@oracle
@pytest.mark.parametrize("history", ["rows", "pingpong"])
def test_feddyn_late_histories(history, delay):
    _both(f"feddyn-{history}", _feddyn_case(history, f"feddyn-{history}"), delay)


@oracle
def test_scaffold_two_rounds(delay):
    """The elementwise interpreter's launches: updates, control variates and (round 1) c_glob late."""
    O = _oracle()
    base0, ups = _data()
    _, ctl = _data(N + 2)
    ends = [f"t{i}" for i in range(N)]
    sizes = {e: 100 + 37 * i for i, e in enumerate(ends)}
    counts, total = [sizes[e] for e in ends], sum(sizes.values())
    ora = O.OracleScaffold(k=3)
    ora.save_state(S._PRE, dataset_sizes=sizes)

    def controls(r):
        cs = []
        for i in range(N):
            c = OrderedDict((k, v * 0.1 if v.is_floating_point() else v.clone()) for k, v in ctl[r][i].items())
            c["nbt"] = torch.tensor(9.25 * (i + 1) + r)
            cs.append(c)
        return cs
    w, rounds = _clone(base0), []
    for r in range(2):
        ora.save_state(S._PRE, glob_weights=w)
        before = {"w": _clone(w), "c_glob": _clone(ora.c_glob) if r else None}
        exp = ora.do(_clone(w), _fill([_clone(u) for u in ups[r]], counts, ends=ends), total=total,
                     control_cache=_fill([_clone(c) for c in controls(r)], [0] * N, ends=ends))
        rounds.append((before, {"out": _clone(exp), "c_glob": _clone(ora.c_glob)}))
        w = _clone(exp)

    def case(L):
        opt = make_amd("scaffold", k=3)
        opt.save_state(S._PRE, dataset_sizes=sizes)
        bases = [L.weights(rounds[r][0]["w"], group=r) for r in range(2)]
        cglob = L.weights(rounds[1][0]["c_glob"], group=1)
        srcs = [[L.weights(u, group=r) for u in ups[r]] for r in range(2)]
        csrcs = [[L.weights(c, group=r) for c in controls(r)] for r in range(2)]
        res = {}
        with L.stream():
            for r in range(2):
                if r:
                    opt.c_glob = dict(cglob)
                L.start(group=r)
                opt.save_state(S._PRE, glob_weights=bases[r])       # (may copy the model: behind the reveal)
                with L.call(f"scaffold/r{r}"):
                    out = opt.do(bases[r], _fill([OrderedDict(u) for u in srcs[r]], counts, ends=ends), total=total,
                                 control_cache=_fill([OrderedDict(c) for c in csrcs[r]], [0] * N, ends=ends))
                L.reuse(*srcs[r], *csrcs[r])
                res[f"r{r}/out"], res[f"r{r}/c_glob"] = L.snap(out), L.snap(opt.c_glob)
        L.finish()
        for r in range(2):
            S.assert_bitwise(f"scaffold/r{r}/out", res[f"r{r}/out"], rounds[r][1]["out"])
            S.assert_bitwise(f"scaffold/r{r}/c_glob", res[f"r{r}/c_glob"], rounds[r][1]["c_glob"])
        return res
    _both("scaffold", case, delay)


# ------------------------------------------------------------------ 6. guard, trim, krum
READBACK = ("engine._measure ends with out.cpu(), the one D2H that waits for the stream "
            "(engine.update_stats / update_gram: 'this is a synchronisation point')")


def _records(recs):
    return {"records": OrderedDict([("norm", torch.tensor([r.norm for r in recs], dtype=torch.float64)),
                                    ("scale", torch.tensor([r.scale for r in recs], dtype=torch.float64)),
                                    ("nonfinite", torch.tensor([r.nonfinite for r in recs])),
                                    ("skipped", torch.tensor([r.skipped for r in recs]))])}


@oracle
def test_guard_clip(delay):
    """clip_threshold: stats -> one readback -> scaled reduce.  The threshold lies between the 2nd and
    3rd largest fp64 norm: exactly those two updates are clipped; the model is the oracle's over the
    updates scaled by the recorded scales."""
    O = _oracle()
    base0, ups = _data()
    n_el = sum(base0[k].numel() for k in FLOAT_KEYS)
    norms = sorted((math.sqrt(sum(float((u[k].double() ** 2).sum()) for k in FLOAT_KEYS)), i) for i, u in enumerate(ups[0]))
    clip, clipped = (norms[-3][0] + norms[-2][0]) / 2, {i for _, i in norms[-2:]}

    def case(L):
        opt = make_amd("fedavg", clip_threshold=clip)
        base, srcs = L.weights(base0), [L.weights(u) for u in ups[0]]
        with L.stream():
            L.start()
            with L.call("guard/clip", sync=READBACK):
                out = opt.do(base, _fill([OrderedDict(u) for u in srcs], COUNTS), total=TOTAL)
            L.reuse(*srcs)
            got = L.snap(out)
        L.finish()
        recs = opt.update_stats
        assert [r.end for r in recs] == [f"e{i:02d}" for i in range(N)]
        assert {i for i, r in enumerate(recs) if r.scale < 1.0} == clipped and not any(r.skipped for r in recs)
        assert all(r.nonfinite == 0 and (r.scale == 1.0 or 0.0 < r.scale < 1.0) for r in recs)
        for r, (ref, _) in zip(recs, sorted(norms, key=lambda t: t[1])):
            # an fp64 sum of n_el squares in any order: (n_el + 1) * 2^-53 relative (test_gpu_update_guard.py)
            assert abs(r.norm - ref) <= (n_el + 1) * 2.0 ** -53 * ref, (r.end, r.norm, ref)
        scaled = [OrderedDict((k, O.tmp_tensor(v, r.scale) if v.is_floating_point() else v.clone()) for k, v in u.items())
                  for u, r in zip(ups[0], recs)]
        exp = O.OracleFedAvg().do(_clone(base0), _fill(scaled, COUNTS), total=TOTAL)
        S.assert_bitwise("guard/clip", got, exp)
        return {"out": got, **_records(recs)}
    _both("guard/clip", case, delay)


@oracle
def test_guard_skip_all_nan_update(delay):
    """nonfinite="skip" with update 2 all NaN: it alone is skipped (its non-finite count is every float
    element), the rates come from what is left of ``total``."""
    O = _oracle()
    base0, ups = _data()
    bad = 2
    round0 = [_clone(u) for u in ups[0]]
    for k in FLOAT_KEYS:
        round0[bad][k].fill_(float("nan"))
    n_float = sum(base0[k].numel() for k in FLOAT_KEYS)
    kept = [i for i in range(N) if i != bad]
    exp = O.OracleFedAvg().do(_clone(base0), _fill([_clone(round0[i]) for i in kept], [COUNTS[i] for i in kept],
                                                   ends=[f"e{i:02d}" for i in kept]), total=TOTAL - COUNTS[bad])

    def case(L):
        opt = make_amd("fedavg", nonfinite="skip")
        base, srcs = L.weights(base0), [L.weights(u) for u in round0]
        with L.stream():
            L.start()
            with L.call("guard/skip", sync=READBACK):
                out = opt.do(base, _fill([OrderedDict(u) for u in srcs], COUNTS), total=TOTAL)
            L.reuse(*srcs)
            got = L.snap(out)
        L.finish()
        recs = opt.update_stats
        assert [r.skipped for r in recs] == [i == bad for i in range(N)]
        assert [r.nonfinite for r in recs] == [n_float if i == bad else 0 for i in range(N)]
        assert all(r.scale == 1.0 for r in recs)
        S.assert_bitwise("guard/skip", got, exp)
        return {"out": got, **_records(recs)}
    _both("guard/skip", case, delay)


def test_trim_two(delay):
    """trim=2 over 7 late updates: asynchronous (nothing is read back); tests/trimmed_ref.py::stream."""
    import trimmed_ref as R
    O = _oracle()
    base0, ups = _data()
    exp = OrderedDict()
    for key, t in base0.items():
        if t.is_floating_point():
            exp[key] = R.stream([u[key].reshape(-1) for u in ups[0]], 2, t, t.dtype).view(t.shape)
        else:       # counters: the existing statement with equal weights (engine.trimmed_mean)
            exp[key] = t.clone()
            O.reduce_tensor(exp[key], [u[key] for u in ups[0]], [1.0 / N] * N)

    def case(L):
        opt = make_amd("fedavg", trim=2)
        base, srcs = L.weights(base0), [L.weights(u) for u in ups[0]]
        with L.stream():
            L.start()
            with L.call("trim2"):
                out = opt.do(base, _fill([OrderedDict(u) for u in srcs], COUNTS), total=TOTAL)
            L.reuse(*srcs)
            got = L.snap(out)
        L.finish()
        assert opt.trim_k == 2 and out is base
        for k in exp:
            if exp[k].is_floating_point():
                R.same_bits(f"trim2/{k}", got[k], exp[k])
            else:
                S.assert_bitwise(f"trim2/{k}", {k: got[k]}, {k: exp[k]})
        return {"out": got}
    _both("trim2", case, delay)


@oracle
def test_krum_two(delay):
    """krum=2 over 9 late updates (7 honest, 2 bad, tests/krum_ref.py's honest_bad): the selected set is
    the reference's; the model is the oracle's FedAvg over the selected updates with equal weights."""
    import krum_ref as R
    O = _oracle()
    n, f = 9, 2
    g = torch.Generator().manual_seed(31)
    base0 = OrderedDict([("k0", torch.randn(4099, generator=g)), ("k1", torch.randn(210, generator=g)), ("nbt", torch.tensor(7))])
    ups, honest = R.honest_bad(g, n, f, (4099, 210), torch.float32)
    for i, u in enumerate(ups):
        u["nbt"] = torch.tensor(100 + 37 * i)
    _, ref_sel, _, _ = R.krum(ups, f)
    assert ref_sel == honest
    counts = [5 + i for i in range(n)]
    exp = O.OracleFedAvg().do(_clone(base0), _fill([_clone(ups[i]) for i in ref_sel], [1] * len(ref_sel)), total=n - f)

    def case(L):
        opt = make_amd("fedavg", krum=f)
        base, srcs = L.weights(base0), [L.weights(u) for u in ups]
        with L.stream():
            L.start()
            with L.call("krum2", sync=READBACK):
                out = opt.do(base, _fill([OrderedDict(u) for u in srcs], counts), total=sum(counts))
            L.reuse(*srcs)
            got = L.snap(out)
        L.finish()
        recs = opt.krum_records
        assert [i for i, r in enumerate(recs) if r.selected] == ref_sel
        S.assert_bitwise("krum2", got, exp)
        return {"out": got, "scores": {"s": torch.tensor([r.score for r in recs], dtype=torch.float64)}}
    _both("krum2", case, delay)


# ------------------------------------------------------------------ 7. host-resident everything
@oracle
def test_host_resident_model_state_and_pinned_updates(delay):
    """FedAdam with a pageable host model and host state and pinned (zero-copy) updates.  Only the
    pinned updates can be written late.  The results are read ON THE HOST right after do() returns,
    with no synchronise by the test: the write-back into a host-resident target completes before the
    call returns (engine._Target.writeback), which is also why the delay cannot outlast the call."""
    _, ups = _data()
    rounds = _fedopt_expected("fedadam")
    writeback = "engine._Target.writeback: a host-resident target is complete when the call returns"

    def case(L):
        opt = make_amd("fedadam")
        srcs = [[L.weights(u, "pinned", group=r) for u in ups[r]] for r in range(ROUNDS)]
        res = {}
        with L.stream():
            for r in range(ROUNDS):
                base = _clone(rounds[r][0]["cur"])
                if r:
                    opt.current_weights = _clone(rounds[r][0]["cur"])
                if rounds[r][0]["m"]:
                    opt.m_t, opt.v_t = dict(_clone(rounds[r][0]["m"])), dict(_clone(rounds[r][0]["v"]))
                L.start(group=r)
                with L.call(f"host-all/r{r}", sync=writeback):
                    got = opt.do(base, _fill([OrderedDict(u) for u in srcs[r]], COUNTS), total=TOTAL)
                assert all(not t.is_cuda for t in base.values())
                res[f"r{r}/avg"] = OrderedDict((k, v.clone()) for k, v in base.items())      # host reads, at once
                S.same_bits(f"host-all/r{r}/avg", res[f"r{r}/avg"], rounds[r][1]["avg"])
                res[f"r{r}/cur"] = L.snap(got)
        L.finish()
        for r in range(ROUNDS):
            S.same_bits(f"host-all/r{r}/cur", res[f"r{r}/cur"], rounds[r][1]["cur"])
        return res
    _both("host-all", case, delay)


# ------------------------------------------------------------------ 8. egress
@oracle
def test_egress_of_a_late_model(delay):
    """A model produced late on ``s`` (FedAvg over late updates), serialised under ``s`` and decoded on
    the host at once: MessageEncoder.encode synchronises the current stream before it returns."""
    from flame_amd import egress, ingest
    base0, ups = _data()
    exp = _fedavg_expected()

    def case(L):
        base, srcs = L.weights(base0), [L.weights(u) for u in ups[0]]
        enc = egress.MessageEncoder(ring=2)
        with L.stream():
            L.start()
            with L.call("egress/do"):
                out = make_amd("fedavg").do(base, _fill([OrderedDict(u) for u in srcs], COUNTS), total=TOTAL)
            with L.call("egress", sync="egress.MessageEncoder.encode: 'the payload is complete when encode returns'"):
                payload = enc.encode({"weights": out, "round": 3})
            msg = ingest.decode(bytes(payload))
        L.finish()
        assert msg["round"] == 3 and list(msg["weights"]) == list(exp)
        got = OrderedDict((k, v.clone()) for k, v in msg["weights"].items())
        S.assert_bitwise("egress", got, exp)
        return {"out": got}
    _both("egress", case, delay)


# ------------------------------------------------------------------ 9. stream hand-over
class _Streams:
    """Round 0 under s1, ``s2.wait_stream(s1)``, round 1 under s2, ``default.wait_stream(s2)``, round 2
    on the default stream -- one optimizer object throughout (engine._STREAMS, the staging side
    stream, events recorded under one stream and consumed under the next)."""

    def __init__(self):
        self.s = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV), torch.cuda.default_stream(torch.device(DEV))]


class _round_stream:
    def __init__(self, L, streams, r):
        self.L, self.streams, self.r = L, streams, r

    def __enter__(self):
        L = self.L
        if L.ready or self.streams is None:
            self.cm = L.stream()
        else:
            if not L.synced:
                torch.cuda.synchronize()
                L.synced = True
            st = self.streams.s[self.r]
            if self.r:
                st.wait_stream(self.streams.s[self.r - 1])
            L.s = st
            self.cm = torch.cuda.stream(st)
        return self.cm.__enter__()

    def __exit__(self, *exc):
        return self.cm.__exit__(*exc)


def _finish(L, streams):
    if streams is not None and not L.ready:
        assert not L.groups
        torch.cuda.synchronize()
    else:
        L.finish()


@oracle
@pytest.mark.parametrize("which", ["fedadam", "feddyn-pingpong"])
def test_stream_hand_over(which, delay):
    def make(L):
        streams = None if L.ready else _Streams()
        if which == "fedadam":
            return _fedopt_case("fedadam", "handover/fedadam", streams)(L)
        return _feddyn_case("pingpong", "handover/feddyn-pingpong", streams)(L)
    _both(f"handover/{which}", make, delay)
