"""GPU: MXFP4 updates (packed e2m1 elements, one E8M0 scale per 32) into an fp32 model in one reduction
launch (flame_agg_reduce_mxfp4), bit for bit what the fp32 reduction gives over ``mx.dequantize(update)``.

The checker is the torch-CPU restatement of tests/uplink16_case.py over the dequantised fp32 updates
-- ``tmp = v * rate`` in fp32, ``acc += tmp`` in fp32 -- and ``mx.dequantize`` itself is checked
against an integer-arithmetic restatement by tests/test_mxfp4_ref.py.

* Shapes around the lane's 32 elements (= the block) and the 8,192-element chunk, client counts around
  the unroll of 4, several keys per launch, updates on the device, in pinned and in pageable host
  memory; client bytes 1 and 4 bytes off alignment, a base 4 bytes off, scales at an odd address.
* All 256 x 256 (packed byte, scale byte) pairs under eight rates and six bases: the test that decides
  whether v_cvt_scalef32_pk_f32_fp4 may decode the elements.
* An odd numel whose pad nibble is 0xF, with poisoned bytes behind it.
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
from large_case import Launches
from oracle import consult

pytestmark = [pytest.mark.gpu]
oracle = pytest.mark.oracle

DEV = "cuda:0"
WHO = "flame_agg_reduce_mxfp4"
UNROLL = 4
NUMELS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 2 * 8192 + 37]
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


def _bytes(numels, nc):
    return sum(nc * -(-n // 2) + 8 * n + nc * -(-n // 32) for n in numels)


# ---------------------------------------------------------------------------- shapes
_DATA = {}


def _data():
    """The fp32 bases, 11 quantised updates over all NUMELS keys (every block at its own magnitude, some
    zeros, a NaN block and an inf), the rates, and the restated result per client count.  Built once and
    never written."""
    from flame_amd import mx
    consult.note()          # the restated results are shared: every test that takes them consults the checker
    if not _DATA:
        g = torch.Generator().manual_seed(812)
        rates = (torch.rand(max(NCL), generator=g, dtype=torch.float64) / 8).tolist()
        base = OrderedDict((k, torch.randn(n, generator=g)) for k, n in zip(KEYS, NUMELS))
        ups = []
        for i in range(max(NCL)):
            w = OrderedDict()
            for k, n in zip(KEYS, NUMELS):
                mag = torch.exp2(torch.randint(-30, 12, (-(-n // 32),), generator=g).float()).repeat_interleave(32)[:n]
                x = torch.randn(n, generator=g) * mag * (0.1 + i)
                x[torch.rand(n, generator=g) < 0.02] = 0.0
                if i == 2 and n > 40:
                    x[37] = float("nan")
                    x[5] = float("inf")
                w[k] = x
            ups.append(mx.quantize(w, "e2m1"))
        deq = [mx.dequantize(u) for u in ups]
        exp = {nc: OrderedDict((k, restate(base[k], [d[k] for d in deq[:nc]], rates[:nc])) for k in KEYS) for nc in NCL}
        _DATA["all"] = (base, ups, rates, exp, deq)
    return _DATA["all"]


def _placed(u, where):
    return u.to(DEV) if where == "device" else u.pin_memory() if where == "pinned" else u


@oracle
@pytest.mark.parametrize("where", ["device", "pinned", "pageable"])
def test_accumulate_shapes(where):
    """Every numel as one segment of ONE launch per client count."""
    from flame_amd import engine
    base, ups, rates, exp, _ = _data()
    placed = [_placed(u, where) for u in ups]
    for nc in NCL:
        agg = S.to_dev(base, DEV)
        with Launches() as ln:
            engine.accumulate(agg, list(zip(placed[:nc], rates[:nc])))
        torch.cuda.synchronize()
        assert ln.names == [WHO], ln.names
        assert ln.bytes[WHO] == _bytes(NUMELS, nc)
        S.same_bits(f"{where}/n={nc}", agg, exp[nc])


def _off(t, by):
    """A device view of ``t``'s bytes that starts ``by`` bytes past a fresh allocation."""
    raw = t.contiguous().view(-1).view(torch.uint8)
    buf = torch.empty(raw.numel() + 16, dtype=torch.uint8, device=DEV)
    v = buf[by:by + raw.numel()]
    v.copy_(raw)
    assert v.data_ptr() % 16 == by
    return v.view(t.dtype).view(t.shape)


@oracle
@pytest.mark.parametrize("layout", ["client_off_1", "client_off_4", "base_misaligned", "scales_odd"])
def test_reduce_misaligned(layout):
    from flame_amd import engine
    base, ups, rates, exp, _ = _data()
    nc = UNROLL + 1
    by = {"client_off_1": 1, "client_off_4": 4}.get(layout)
    outs = [_off(base[k], 4) if layout == "base_misaligned" else base[k].to(DEV, copy=True) for k in KEYS]
    rows = [[_off(u[k], by) if by else u.to(DEV)[k] for u in ups[:nc]] for k in KEYS]
    bsc = [[_off(u.scales[k], 1) if layout == "scales_odd" else u.scales[k].to(DEV) for u in ups[:nc]] for k in KEYS]
    with Launches() as ln:
        engine.reduce_(outs, outs, rows, rates[:nc], block_scales=bsc)
    torch.cuda.synchronize()
    assert ln.names == [WHO], ln.names
    S.same_bits(layout, dict(zip(KEYS, outs)), exp[nc])


# ---------------------------------------------------------------------------- every (byte, scale) pair
RATES = [1.0, 1.0 / 3.0, 0.75, 1e-3, 3.0, -0.5, 0.0, 2.0 ** -20]
BASES = [0.0, -0.0, 1.0, -1e-30, 3e38, float("inf")]


@oracle
def test_every_byte_scale_pair():
    """All 256 x 256 (packed byte, scale byte) pairs, so every code in both nibble positions beside every
    neighbour under every scale: 131,072 elements as 4,096 blocks (block b holds scale byte b // 16 and
    the packed bytes 16 (b % 16) .. + 15), three clients holding block permutations of them; one launch
    per rate triple (every rate is the first client's once), one segment per base.  Covers both signed
    zeros, scale bytes 0 and 255, products that are fp32 subnormals, products that overflow and a base
    that overflows."""
    from flame_amd import engine, mx
    g = torch.Generator().manual_seed(6)
    blocks = torch.arange(4096)
    q0 = (((blocks % 16) * 16).unsqueeze(1) + torch.arange(16).unsqueeze(0)).to(torch.uint8)        # [4096, 16]
    s0 = (blocks // 16).to(torch.uint8)
    n = 4096 * 32
    clients = []
    for i in range(3):
        perm = blocks if i == 0 else torch.randperm(4096, generator=g)
        clients.append(mx.MXWeights({"x": q0[perm].reshape(-1).contiguous().view(mx.PACKED)}, {"x": s0[perm].contiguous()},
                                    shapes={"x": (n,)}))
    pairs = set(zip(clients[1]["x"].view(torch.uint8).tolist(), clients[1].scales["x"].repeat_interleave(16).tolist()))
    assert len(pairs) == 65536
    deq = [mx.dequantize(c)["x"] for c in clients]
    assert deq[0].shape == (n,)
    dev = [c.to(DEV) for c in clients]
    keys = [f"base{j}" for j in range(len(BASES))]
    for i in range(len(RATES)):
        rates = [RATES[i], RATES[(i + 1) % 8], RATES[(i + 3) % 8]]
        outs = [torch.full((n,), b, dtype=torch.float32, device=DEV) for b in BASES]
        engine.reduce_(outs, outs, [[c["x"] for c in dev]] * len(BASES), rates,
                       block_scales=[[c.scales["x"] for c in dev]] * len(BASES))
        torch.cuda.synchronize()
        exp = [restate(torch.full((n,), b, dtype=torch.float32), deq, rates) for b in BASES]
        S.same_bits(f"rates={rates}", dict(zip(keys, outs)), dict(zip(keys, exp)))


# ---------------------------------------------------------------------------- the pad nibble
@oracle
@pytest.mark.parametrize("numel", [33, 8192 + 4097])
def test_pad_nibble_and_what_lies_behind_it_mean_nothing(numel):
    """An odd numel: the last byte's high nibble set to 0xF and every byte behind the update poisoned
    (0xFF: code 15 twice; as a scale byte a NaN) gives the bits of the run with the nibble 0; nothing
    behind the last output element is written."""
    from flame_amd import engine, mx
    g = torch.Generator().manual_seed(numel)
    nc, nb, ns = UNROLL + 1, (numel + 1) // 2, -(-numel // 32)
    ups = [mx.quantize({"x": torch.randn(numel, generator=g) * (i + 1)}, "e2m1") for i in range(nc)]
    rates = [0.5 / (i + 1) for i in range(nc)]
    base = torch.randn(numel, generator=g)
    want = restate(base, [mx.dequantize(u)["x"] for u in ups], rates)

    def run(pad):
        rows, bsc = [], []
        for u in ups:
            q = torch.full((nb + 64,), 0xFF, dtype=torch.uint8)
            q[:nb] = u["x"].view(torch.uint8)
            assert q[nb - 1] >> 4 == 0
            q[nb - 1] |= pad << 4
            s = torch.full((ns + 64,), 0xFF, dtype=torch.uint8)
            s[:ns] = u.scales["x"]
            rows.append(q.to(DEV)[:nb].view(mx.PACKED))
            bsc.append(s.to(DEV)[:ns])
        buf = torch.full((numel + 64,), -7.0, device=DEV)
        buf[:numel] = base.to(DEV)
        out = buf[:numel]
        engine.reduce_([out], [out], [rows], rates, block_scales=[bsc])
        torch.cuda.synchronize()
        assert bool((buf[numel:] == -7.0).all())
        return out.cpu()
    zero, ones = run(0), run(0xF)
    S.same_bits(f"pad 0/{numel}", {"x": zero}, {"x": want})
    S.same_bits(f"pad F/{numel}", {"x": ones}, {"x": zero})


# ---------------------------------------------------------------------------- scaled
@oracle
def test_scaled():
    from flame_amd import engine
    base, ups, rates, exp, deq = _data()
    nc = UNROLL + 1
    scales = [[1.0, 0.5, 1.0 / 3.0, 1e-4][i % 4] for i in range(nc)]
    dev = [u.to(DEV) for u in ups[:nc]]
    agg = S.to_dev(base, DEV)
    with Launches() as ln:
        engine.accumulate(agg, list(zip(dev, rates[:nc])), scales=scales)
    torch.cuda.synchronize()
    assert ln.names == [WHO], ln.names
    want = OrderedDict((k, restate(base[k], [d[k] for d in deq[:nc]], rates[:nc], scales)) for k in KEYS)
    S.same_bits("scaled", agg, want)
    # all-ones scales: the scaled instantiation gives the plain launch's bits
    ones = S.to_dev(base, DEV)
    engine.accumulate(ones, list(zip(dev, rates[:nc])), scales=[1.0] * nc)
    torch.cuda.synchronize()
    S.same_bits("ones", ones, exp[nc])


# ---------------------------------------------------------------------------- through the classes
def _model_round(g, n=9):
    """An fp32 model with a 2-D key of odd numel and an int64 counter; updates quantised but for ``f``
    (below ``min_numel``)."""
    from flame_amd import mx
    base = OrderedDict([("w1", torch.randn(8193, generator=g)), ("w2", torch.randn(3, 4096 + 5, generator=g)),
                        ("f", torch.randn(33, generator=g)), ("nbt", torch.tensor(7))])
    ups = [mx.quantize(OrderedDict([("w1", torch.randn(8193, generator=g) * 0.02 * (i + 1)),
                                    ("w2", torch.randn(3, 4096 + 5, generator=g) * 0.02 * (i + 1)),
                                    ("f", torch.randn(33, generator=g) * 0.02), ("nbt", torch.tensor(i))]), "e2m1", min_numel=64)
           for i in range(n)]
    assert all(sorted(u.scales) == ["w1", "w2"] and u.shapes["w2"] == (3, 4101) and u["w2"].shape == (6152,) for u in ups)
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
def test_do_equals_the_dequantised_round(sort, kw):
    """One ``do`` on MXWeights == the same ``do`` on ``dequantize``d fp32 updates; without noise also the
    restatement.  The MX keys are one launch, ``f`` and ``nbt`` keep theirs."""
    from flame_amd import mx
    base, ups, counts = _model_round(torch.Generator().manual_seed(41))
    total = sum(counts)
    deq = [mx.dequantize(u) for u in ups]
    ref = make_amd(sort, **kw).do(S.to_dev(base, DEV), _cache(deq, counts), total=total)
    with Launches() as ln:
        got = make_amd(sort, **kw).do(S.to_dev(base, DEV), _cache(ups, counts), total=total)
    torch.cuda.synchronize()
    assert ln.count(WHO) == 1 and ln.elementwise() == 0 and ln.count("flame_agg_reduce_mx") == 0, ln.names
    assert ln.count("flame_agg_reduce") == (3 if "noise_factor" in kw else 2), ln.names     # f, nbt (+ the noise)
    assert got["w2"].shape == (3, 4101)
    S.same_bits(f"{sort} vs fp32", got, S.to_cpu(ref))
    want = _restate_model(base, deq, [c / total for c in counts])
    if "noise_factor" not in kw:
        S.same_bits(f"{sort} vs restated", got, want)


@oracle
@pytest.mark.parametrize("where", ["device", "pageable"])
def test_fedavg_deferred_flush(where):
    """FedAvg(defer=True): eager arrivals queued, one flush when the result is read; pageable host
    updates are what ``cloudpickle.loads`` hands over."""
    from flame_amd import mx
    base, ups, counts = _model_round(torch.Generator().manual_seed(42), n=6)
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
    assert ln.count(WHO) == 1 and ln.elementwise() == 0, ln.names
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
    fused: the MXFP4 reduction, then the adaptive step with no clients."""
    from flame_amd import mx
    g = torch.Generator().manual_seed(43)
    n, counts = 5, [4, 9, 2, 7, 3]
    base, _, _ = _model_round(g, n=1)
    per_round = [_model_round(g, n=n)[1] for r in range(3)]
    deq = [[mx.dequantize(u) for u in ws] for ws in per_round]
    exp = _fedopt_rounds(sort, deq, counts, base, n)
    with Launches() as ln:
        got = _fedopt_rounds(sort, per_round, counts, base, n)
    assert ln.count(WHO) == 3 and ln.count("flame_fedopt_reduce_adapt") >= 2, ln.names
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
    """One FedAvg round of MXFP4 updates with every input poisoned until late on a stream of its own:
    asynchronous, bitwise the restatement and the default-stream run."""
    from flame_amd import mx
    base0, ups, counts = _model_round(torch.Generator().manual_seed(44), n=7)
    total = sum(counts)
    want = _restate_model(base0, [mx.dequantize(u) for u in ups], [c / total for c in counts])

    def late(L, u):
        # float4 / uint8 buffers are poisoned and revealed through int8 views of the same bytes
        w = OrderedDict((k, L.tensor(v.view(torch.int8)).view(v.dtype) if k in u.scales else L.tensor(v)) for k, v in u.items())
        return mx.MXWeights(w, {k: L.tensor(s.view(torch.int8)).view(torch.uint8) for k, s in u.scales.items()}, shapes=u.shapes)

    def case(L):
        opt = make_amd("fedavg")
        base, srcs = L.weights(base0), [late(L, u) for u in ups]
        cache = S.SortedCache()
        for i, (u, c) in enumerate(zip(srcs, counts)):
            cache[f"e{i:02d}"] = S.TR(u, c)
        with L.stream():
            L.start()
            with L.call("mxfp4/fedavg"):
                out = opt.do(base, cache, total=total)
            # (torch cannot fill a float4 tensor: the element buffers are handed over as their int8 views)
            views = [OrderedDict((k, v.view(torch.int8) if v.dtype == mx.PACKED else v) for k, v in u.items()) for u in srcs]
            for u in srcs:
                dict.clear(u)
            L.reuse(*views, *[u.scales for u in srcs])
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
    SC.assert_same("mxfp4", ready, late_res)
