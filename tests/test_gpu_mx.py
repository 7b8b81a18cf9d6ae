"""GPU: MXFP8 updates (float8 elements, one E8M0 scale per 32) into an fp32 model in one reduction
launch per element format (flame_agg_reduce_mx).

The oracle is the torch-CPU restatement of the reference's two statements (``tmp = v * rate;
base += tmp``, tests/uplink16_case.py ``restate``) over ``mx.dequantize(update)`` on the CPU -- the
contract's definition of an MX update's value.  Comparisons are ``scenarios.same_bits``: bitwise, signs
of zero included, a NaN equals a NaN.

* Shapes around the lane's 16 elements, the 32-element block and the 4,096-element chunk, client counts
  around the unroll of 8, both formats, several keys per launch, updates on the device, in pinned and
  in pageable host memory; a client tensor and a base 4 bytes off alignment, scales at an odd address.
* All 256 x 256 (element, scale) byte pairs of each format under eight rates and six bases: the test
  that decides whether v_cvt_pk_f32_fp8 / _bf8 may decode the elements.
* Clip scales against the restatement; all-ones scales against the unscaled launch.
* Through the classes: FedAvg, FedProx, FedAvg(noise_factor=), FedAvg(defer=True) and three rounds of
  each FedOPT sort give the bits of the same call on dequantised fp32 updates.
* One case on a non-default stream with late inputs (tests/stream_case.py).
"""
from collections import OrderedDict
from copy import deepcopy

import pytest
import torch

import scenarios as S
import stream_case as SC
import uplink16_case as U
from oracle import consult

pytestmark = [pytest.mark.gpu]
oracle = pytest.mark.oracle

DEV = "cuda:0"
FMTS = ["e4m3", "e5m2"]
UNROLL = 8
NUMELS = [1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 2 * 4096 + 37]
NCL = [1, 2, UNROLL - 1, UNROLL, UNROLL + 1, 2 * UNROLL + 3]
KEYS = [f"k{n}" for n in NUMELS]


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()
    torch.empty(1, device=DEV)


def make_amd(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def restate(base, clients, rates, scales=None):
    """The torch-CPU checker of this file (counted as a consultation, as oracle/torch_cpu.py's loops are)."""
    consult.note()
    return U.restate(base, clients, rates, scales)


class Launches:
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
        self.bytes = {ev[0]: ev[3] for ev in self.events}
        return False

    def count(self, name):
        return sum(1 for n in self.names if n == name)

    def elementwise(self):
        return sum(1 for n in self.names if n.startswith("flame_elementwise"))


# ---------------------------------------------------------------------------- shapes
_DATA = {}


def _data(fmt):
    """The fp32 bases, 19 quantised updates over all NUMELS keys (every block at its own magnitude, some
    zeros and NaNs), the rates, and the restated result per client count.  Built once per format and
    never written."""
    from flame_amd import mx
    consult.note()          # the restated results are shared: every test that takes them consults the checker
    if fmt not in _DATA:
        g = torch.Generator().manual_seed(800 + FMTS.index(fmt))
        rates = (torch.rand(max(NCL), generator=g, dtype=torch.float64) / 8).tolist()
        base = OrderedDict((k, torch.randn(n, generator=g)) for k, n in zip(KEYS, NUMELS))
        ups = []
        for i in range(max(NCL)):
            w = OrderedDict()
            for k, n in zip(KEYS, NUMELS):
                mag = torch.exp2(torch.randint(-30, 12, (-(-n // 32),), generator=g).float()).repeat_interleave(32)[:n]
                x = torch.randn(n, generator=g) * mag * (0.1 + i)
                x[torch.rand(n, generator=g) < 0.02] = 0.0
                if i == 3 and n > 40:
                    x[37] = float("nan")
                    x[5] = float("inf")
                w[k] = x
            ups.append(mx.quantize(w, fmt))
        deq = [mx.dequantize(u) for u in ups]
        exp = {nc: OrderedDict((k, restate(base[k], [d[k] for d in deq[:nc]], rates[:nc])) for k in KEYS) for nc in NCL}
        _DATA[fmt] = (base, ups, rates, exp, deq)
    return _DATA[fmt]


def _placed(u, where):
    return u.to(DEV) if where == "device" else u.pin_memory() if where == "pinned" else u


@oracle
@pytest.mark.parametrize("where", ["device", "pinned", "pageable"])
@pytest.mark.parametrize("fmt", FMTS)
def test_accumulate_shapes(fmt, where):
    """Every numel as one segment of ONE launch per client count."""
    from flame_amd import engine
    base, ups, rates, exp, _ = _data(fmt)
    placed = [_placed(u, where) for u in ups]
    for nc in NCL:
        agg = S.to_dev(base, DEV)
        with Launches() as ln:
            engine.accumulate(agg, list(zip(placed[:nc], rates[:nc])))
        torch.cuda.synchronize()
        assert ln.names == ["flame_agg_reduce_mx"], ln.names
        assert ln.bytes["flame_agg_reduce_mx"] == sum(n * (nc + 8) + nc * -(-n // 32) for n in NUMELS)
        S.same_bits(f"{fmt}/{where}/n={nc}", agg, exp[nc])


def _off(t, by):
    """A device view of ``t``'s bytes that starts ``by`` bytes past a fresh allocation."""
    raw = t.contiguous().view(-1).view(torch.uint8)
    buf = torch.empty(raw.numel() + 16, dtype=torch.uint8, device=DEV)
    v = buf[by:by + raw.numel()]
    v.copy_(raw)
    assert v.data_ptr() % 16 == by
    return v.view(t.dtype).view(t.shape)


@oracle
@pytest.mark.parametrize("layout", ["client_misaligned", "base_misaligned", "scales_odd"])
@pytest.mark.parametrize("fmt", FMTS)
def test_reduce_misaligned(fmt, layout):
    from flame_amd import engine
    base, ups, rates, exp, _ = _data(fmt)
    nc = UNROLL + 1
    outs = [_off(base[k], 4) if layout == "base_misaligned" else base[k].to(DEV, copy=True) for k in KEYS]
    rows = [[_off(u[k], 4) if layout == "client_misaligned" else u[k].to(DEV) for u in ups[:nc]] for k in KEYS]
    bsc = [[_off(u.scales[k], 1) if layout == "scales_odd" else u.scales[k].to(DEV) for u in ups[:nc]] for k in KEYS]
    with Launches() as ln:
        engine.reduce_(outs, outs, rows, rates[:nc], block_scales=bsc)
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_mx"], ln.names
    S.same_bits(f"{fmt}/{layout}", dict(zip(KEYS, outs)), exp[nc])


# ---------------------------------------------------------------------------- every (element, scale) pair
RATES = [1.0, 1.0 / 3.0, 0.75, 1e-3, 3.0, -0.5, 0.0, 2.0 ** -20]
BASES = [0.0, -0.0, 1.0, -1e-30, 3e38, float("inf")]


@oracle
@pytest.mark.parametrize("fmt", FMTS)
def test_every_element_scale_pair(fmt):
    """All 256 x 256 (element byte, scale byte) pairs: 65,536 elements as 2,048 blocks (block b holds
    scale byte b // 8 and element bytes 32 (b % 8) .. + 31), three clients holding block permutations
    of them; one launch per rate triple (every rate is the first client's once), one segment per
    base.  Covers both signed zeros, every subnormal and NaN byte, scale bytes 0 and 255, products that
    are fp32 subnormals and a base that overflows."""
    from flame_amd import engine, mx
    g = torch.Generator().manual_seed(6)
    dt = mx.FORMATS[fmt][0]
    blocks = torch.arange(2048)
    q0 = (((blocks % 8) * 32).unsqueeze(1) + torch.arange(32).unsqueeze(0)).to(torch.uint8)       # [2048, 32]
    s0 = (blocks // 8).to(torch.uint8)
    clients = []
    for i in range(3):
        perm = blocks if i == 0 else torch.randperm(2048, generator=g)
        clients.append(mx.MXWeights({"x": q0[perm].reshape(-1).contiguous().view(dt)}, {"x": s0[perm].contiguous()}))
    pairs = set(zip(clients[1]["x"].view(torch.uint8).tolist(), clients[1].scales["x"].repeat_interleave(32).tolist()))
    assert len(pairs) == 65536
    deq = [mx.dequantize(c)["x"] for c in clients]
    dev = [c.to(DEV) for c in clients]
    keys = [f"base{j}" for j in range(len(BASES))]
    for i in range(len(RATES)):
        rates = [RATES[i], RATES[(i + 1) % 8], RATES[(i + 3) % 8]]
        outs = [torch.full((65536,), b, dtype=torch.float32, device=DEV) for b in BASES]
        engine.reduce_(outs, outs, [[c["x"] for c in dev]] * len(BASES), rates,
                       block_scales=[[c.scales["x"] for c in dev]] * len(BASES))
        torch.cuda.synchronize()
        exp = [restate(torch.full((65536,), b, dtype=torch.float32), deq, rates) for b in BASES]
        S.same_bits(f"{fmt}/rates={rates}", dict(zip(keys, outs)), dict(zip(keys, exp)))


# ---------------------------------------------------------------------------- scaled
@oracle
@pytest.mark.parametrize("fmt", FMTS)
def test_scaled(fmt):
    from flame_amd import engine
    base, ups, rates, exp, deq = _data(fmt)
    nc = UNROLL + 1
    scales = [[1.0, 0.5, 1.0 / 3.0, 1e-4][i % 4] for i in range(nc)]
    dev = [u.to(DEV) for u in ups[:nc]]
    agg = S.to_dev(base, DEV)
    with Launches() as ln:
        engine.accumulate(agg, list(zip(dev, rates[:nc])), scales=scales)
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_mx"], ln.names
    want = OrderedDict((k, restate(base[k], [d[k] for d in deq[:nc]], rates[:nc], scales)) for k in KEYS)
    S.same_bits(f"scaled/{fmt}", agg, want)
    # all-ones scales: the scaled instantiation gives the plain launch's bits
    ones = S.to_dev(base, DEV)
    engine.accumulate(ones, list(zip(dev, rates[:nc])), scales=[1.0] * nc)
    torch.cuda.synchronize()
    S.same_bits(f"ones/{fmt}", ones, exp[nc])


# ---------------------------------------------------------------------------- through the classes
def _model_round(g, fmt, n=9):
    """An fp32 model with an int64 counter; updates quantised but for ``f`` (below ``min_numel``)."""
    from flame_amd import mx
    base = OrderedDict([("w1", torch.randn(4097, generator=g)), ("w2", torch.randn(3, 4096 + 5, generator=g)),
                        ("f", torch.randn(33, generator=g)), ("nbt", torch.tensor(7))])
    ups = [mx.quantize(OrderedDict([("w1", torch.randn(4097, generator=g) * 0.02 * (i + 1)),
                                    ("w2", torch.randn(3, 4096 + 5, generator=g) * 0.02 * (i + 1)),
                                    ("f", torch.randn(33, generator=g) * 0.02), ("nbt", torch.tensor(i))]), fmt, min_numel=64)
           for i in range(n)]
    assert all(sorted(u.scales) == ["w1", "w2"] for u in ups)
    return base, ups, [5 + 3 * i for i in range(n)]


def _restate_model(base, deq, rates):
    return OrderedDict((k, restate(b, [d[k] for d in deq], rates)) for k, b in base.items())


def _cache(ws, counts, device=DEV):
    cache = S.SortedCache()
    for i, (w, c) in enumerate(zip(ws, counts)):
        cache[f"e{i:02d}"] = S.TR(w.to(device) if hasattr(w, "scales") else S.to_dev(w, device), c)
    return cache


@oracle
@pytest.mark.parametrize("sort,kw", [("fedavg", {}), ("fedprox", {"mu": 0.01}),
                                     ("fedavg", {"noise_factor": 0.05, "noise_seed": 11})],
                         ids=["fedavg", "fedprox", "fedavg-noise"])
@pytest.mark.parametrize("fmt", FMTS)
def test_do_equals_the_dequantised_round(fmt, sort, kw):
    """One ``do`` on MXWeights == the same ``do`` on ``dequantize``d fp32 updates; without noise also the
    restatement.  The MX keys are one launch, ``f`` and ``nbt`` keep theirs."""
    from flame_amd import mx
    base, ups, counts = _model_round(torch.Generator().manual_seed(41), fmt)
    total = sum(counts)
    deq = [mx.dequantize(u) for u in ups]
    ref = make_amd(sort, **kw).do(S.to_dev(base, DEV), _cache(deq, counts), total=total)
    with Launches() as ln:
        got = make_amd(sort, **kw).do(S.to_dev(base, DEV), _cache(ups, counts), total=total)
    torch.cuda.synchronize()
    assert ln.count("flame_agg_reduce_mx") == 1 and ln.elementwise() == 0, ln.names
    assert ln.count("flame_agg_reduce") == (3 if "noise_factor" in kw else 2), ln.names     # f, nbt (+ the noise)
    S.same_bits(f"{sort}/{fmt} vs fp32", got, S.to_cpu(ref))
    want = _restate_model(base, deq, [c / total for c in counts])
    if "noise_factor" not in kw:
        S.same_bits(f"{sort}/{fmt} vs restated", got, want)


@oracle
@pytest.mark.parametrize("where", ["device", "pageable"])
def test_fedavg_deferred_flush(where):
    """FedAvg(defer=True): eager arrivals queued, one flush when the result is read; pageable host
    updates are what ``cloudpickle.loads`` hands over."""
    from flame_amd import mx
    base, ups, counts = _model_round(torch.Generator().manual_seed(42), "e4m3", n=6)
    opt = make_amd("fedavg", defer=True)
    dev_base = S.to_dev(base, DEV)
    cache = S.SortedCache()
    want, running, out = base, 0, None
    for i, (u, c) in enumerate(zip(ups, counts)):
        running += c
        cache[f"e{i:02d}"] = S.TR(u.to(DEV) if where == "device" else u, c)
        out = opt.do(dev_base, cache, total=running)
        want = _restate_model(want, [mx.dequantize(u)], [c / running])
    with Launches() as ln:
        got = OrderedDict((k, out[k]) for k in out)        # the read runs the queue
    torch.cuda.synchronize()
    assert ln.count("flame_agg_reduce_mx") == 1 and ln.elementwise() == 0, ln.names
    S.same_bits(f"deferred/{where}", got, want)


def _fedopt_rounds(sort, per_round, counts, weights0, n):
    opt = make_amd(sort, beta_1=0.9, beta_2=0.99, eta=0.1, tau=1e-3)
    weights = S.to_dev(weights0, DEV)
    res = []
    for r, ws in enumerate(per_round):
        weights = opt.do(deepcopy(weights), _cache(ws, counts), total=sum(counts), num_trainers=n)
        res.append((f"r{r}/cur", S.to_cpu(weights)))
        res.append((f"r{r}/avg", S.to_cpu(opt.agg_weights)))
        if opt.m_t is not None:
            res.append((f"r{r}/m", S.to_cpu(opt.m_t)))
            res.append((f"r{r}/v", S.to_cpu(opt.v_t)))
    return res


@oracle
@pytest.mark.parametrize("sort", U.SORTS)
def test_fedopt_rounds_equal_the_dequantised_rounds(sort):
    """Three rounds on MXWeights against the same class fed dequantised updates: ``agg_weights`` bitwise
    (and the restatement's), the rest under the contract of the fp32 FedOPT fixtures.  The keys are
    fused: the MX reduction, then the adaptive step with no clients."""
    from flame_amd import mx
    g = torch.Generator().manual_seed(43)
    n, counts = 5, [4, 9, 2, 7, 3]
    base, _, _ = _model_round(g, "e4m3", n=1)
    per_round = [_model_round(g, FMTS[r % 2], n=n)[1] for r in range(3)]
    deq = [[mx.dequantize(u) for u in ws] for ws in per_round]
    exp = _fedopt_rounds(sort, deq, counts, base, n)
    with Launches() as ln:
        got = _fedopt_rounds(sort, per_round, counts, base, n)
    assert ln.count("flame_agg_reduce_mx") == 3 and ln.count("flame_fedopt_reduce_adapt") >= 2, ln.names
    assert [l for l, _ in got] == [l for l, _ in exp]
    for (label, a), (_, b) in zip(got, exp):
        if label.endswith("/avg"):
            S.same_bits(f"{sort}:{label}", a, b)
    U.check_fedopt(sort, [(label, a, b) for (label, a), (_, b) in zip(got, exp)])
    # round 0's average against the restatement: base + the dequantised updates
    want = _restate_model(base, deq[0], [c / sum(counts) for c in counts])
    S.same_bits(f"{sort}: r0/avg restated", dict(got)["r0/avg"], want)


# ---------------------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def delay():
    d = SC.Delay()
    yield d
    d.free()


@oracle
def test_round_on_a_late_stream(delay):
    """One FedAvg round of MX updates with every input poisoned until late on a stream of its own:
    asynchronous, bitwise the restatement and the default-stream run."""
    from flame_amd import mx
    base0, ups, counts = _model_round(torch.Generator().manual_seed(44), "e5m2", n=7)
    total = sum(counts)
    want = _restate_model(base0, [mx.dequantize(u) for u in ups], [c / total for c in counts])

    def late(L, u):
        # float8 / uint8 buffers are poisoned and revealed through int8 views of the same bytes
        w = OrderedDict((k, L.tensor(v.view(torch.int8)).view(v.dtype) if k in u.scales else L.tensor(v)) for k, v in u.items())
        return mx.MXWeights(w, {k: L.tensor(s.view(torch.int8)).view(torch.uint8) for k, s in u.scales.items()})

    def case(L):
        opt = make_amd("fedavg")
        base, srcs = L.weights(base0), [late(L, u) for u in ups]
        cache = S.SortedCache()
        for i, (u, c) in enumerate(zip(srcs, counts)):
            cache[f"e{i:02d}"] = S.TR(u, c)
        with L.stream():
            L.start()
            with L.call("mx/fedavg"):
                out = opt.do(base, cache, total=total)
            L.reuse(*srcs, *[u.scales for u in srcs])
            res = {"out": L.snap(out)}
        L.finish()
        S.same_bits("late", res["out"], want)
        return res
    ready = case(SC.Late(delay, ready=True))
    # a stream of the high-priority pool: torch's default-priority pool hands its streams out round-robin,
    # and which of them a later test of the process gets decides that test's hardware queue
    # (tests/test_gpu_streams.py's pageable-host insert is sensitive to it); this pool has a
    # cursor of its own, so the default one stays where it was
    late_res = case(SC.Late(delay, stream=torch.cuda.Stream(DEV, priority=-1)))
    SC.assert_same("mx", ready, late_res)
