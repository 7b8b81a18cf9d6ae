"""GPU: the MX quantiser (flame_mx_quantize, engine.mx_quantize, MessageEncoder(mx=)) against ``mx.quantize`` on a
CPU copy, by the contract of DESIGN.md §2.  The rounding-boundary test decides the conversion arm a format ships
with; its block exponents stop at 127 - emax: above it the anchor a * 2^(e + emax) is not an fp32."""
import pickle
from collections import OrderedDict

import pytest
import torch

import stream_case as SC
from large_case import Launches
from oracle import consult

pytestmark = [pytest.mark.gpu]
oracle = pytest.mark.oracle
DEV, WHO, POISON, CHUNK = "cuda:0", "flame_mx_quantize", 0xA5, 8192
FMTS = ["e4m3", "e5m2", "e2m1"]
SRCS = [torch.float32, torch.bfloat16, torch.float16]
NUMELS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 37]


def same(label, q, s, x, fmt):
    """Element bytes ``q`` and scale bytes ``s`` are ``mx.quantize``'s of the CPU tensor ``x``, by the contract."""
    from flame_amd import mx
    consult.note()
    w = mx.quantize({"k": x.cpu()}, fmt)
    rq, q = w["k"].view(torch.uint8).reshape(-1), q.cpu().view(torch.uint8).reshape(-1)
    assert torch.equal(s.cpu(), w.scales["k"]), f"{label}: scale bytes differ"
    isnan = lambda b: (b & 0x7F) > {"e4m3": 0x7E, "e5m2": 0x7C, "e2m1": 0xFF}[fmt]      # noqa: E731
    nan = isnan(rq)
    bad = ((q != rq) & ~nan).nonzero().flatten()
    assert bad.numel() == 0, f"{label}: {bad.numel()} element bytes differ, first at {bad[:1].tolist()}"
    assert bool(isnan(q[nan]).all()), f"{label}: a NaN element left as a number"


def _key(n, g, dtype):
    """``n`` values, every block at its own magnitude, some zeros and -0, one NaN, one inf, one all-zero block."""
    mag = torch.exp2(torch.randint(-30, 13, (-(-n // 32),), generator=g).float()).repeat_interleave(32)[:n]
    x = torch.randn(n, generator=g) * mag
    x[torch.rand(n, generator=g) < 0.03] = 0.0
    x[torch.rand(n, generator=g) < 0.02] = -0.0
    if n > 200:
        x[37], x[70], x[101] = float("nan"), float("inf"), float("-inf")
        x[128:160] = 0.0
    return x.to(dtype)


@oracle
@pytest.mark.parametrize("src", SRCS, ids=str)
@pytest.mark.parametrize("fmt", FMTS)
def test_shapes_and_extents(fmt, src):
    """Every numel as one segment of ONE launch, guard bytes behind every output."""
    from flame_amd import engine, mx
    g = torch.Generator().manual_seed(77)
    xs = [_key(n, g, src) for n in NUMELS]
    nq = [engine.mx_out_bytes(fmt, n) for n in NUMELS]
    qs = [torch.full((b + 64,), POISON, dtype=torch.uint8, device=DEV) for b in nq]
    ss = [torch.full((mx.n_blocks(n) + 64,), POISON, dtype=torch.uint8, device=DEV) for n in NUMELS]
    with Launches() as ln:
        engine.mx_quantize_([x.to(DEV) for x in xs], [q[:b] for q, b in zip(qs, nq)],
                            [s[:mx.n_blocks(n)] for s, n in zip(ss, NUMELS)], fmt)
    torch.cuda.synchronize()
    assert ln.names == [WHO], ln.names
    assert ln.bytes[WHO] == sum(n * src.itemsize + b + mx.n_blocks(n) for n, b in zip(NUMELS, nq))
    for n, x, q, s, b in zip(NUMELS, xs, qs, ss, nq):
        same(f"{fmt}/{src}/n={n}", q[:b], s[:mx.n_blocks(n)], x, fmt)     # (an odd e2m1 key's pad nibble is the reference's 0)
        assert bool((q[b:] == POISON).all()) and bool((s[mx.n_blocks(n):] == POISON).all()), f"n={n}: written past the extent"


def _boundary_blocks(fmt):
    """The rounding-boundary input of ``fmt`` (module docstring, ISSUE): fp32 blocks [B, 32]."""
    from flame_amd import mx
    _, emax, fmax = mx.FORMATS[fmt]
    if fmt == "e2m1":
        codes = torch.tensor(mx.E2M1_VALUES[1:8], dtype=torch.float32)
    else:
        b = torch.arange(1, 256, dtype=torch.uint8).view(mx.FORMATS[fmt][0]).float()
        codes = b[torch.isfinite(b) & (b > 0)]
    mid = torch.cat([codes[:1] / 2, (codes[:-1] + codes[1:]) / 2])
    up, down = torch.nextafter(mid, mid.new_tensor(float("inf"))), torch.nextafter(mid, mid.new_tensor(0.0))
    top = torch.tensor([fmax]).float()
    sat = torch.cat([torch.nextafter(top, top * 2), top * torch.tensor([1.03, 1.07, 1.1, 1.14]),
                     torch.nextafter(torch.tensor([2.0 ** (emax + 1)]), top)])
    v = torch.cat([codes, mid, up, down, sat, -codes, -mid, -up, -down, -sat]).double()
    v = torch.cat([v, v[:(-v.numel()) % 31]]).view(-1, 31)
    anchors = [1.0, 1.75 if fmt != "e2m1" else 1.5, float(torch.nextafter(torch.tensor(2.0), torch.tensor(0.0)))]
    es = sorted(set(range(-127, -117)) | set(range(110, 128 - emax)) | set(range(-118, 110, 8)))
    blocks = []
    for i, (e, a) in enumerate((e, a) for e in es for a in anchors):
        blk = torch.empty(v.shape[0], 32, dtype=torch.float64)
        pos = (i + torch.arange(v.shape[0])) % 32                       # the anchor rotates through the block
        rest = torch.ones(v.shape[0], 32, dtype=torch.bool).scatter_(1, pos.view(-1, 1), False)
        blk[rest] = torch.ldexp(v, torch.tensor(e)).reshape(-1)
        blk[~rest] = a * 2.0 ** (e + emax)
        blocks.append(blk)
    sub = torch.zeros(v.shape[0], 32, dtype=torch.float64)              # no anchor: the maximum is an fp32 subnormal
    sub[:, :31] = torch.where(v.abs() < 2, torch.ldexp(v, torch.tensor(-127)), torch.zeros_like(v))
    return torch.cat(blocks + [sub]).float()


@oracle
@pytest.mark.parametrize("fmt", FMTS)
def test_rounding_boundaries(fmt):
    from flame_amd import engine
    x = _boundary_blocks(fmt).reshape(-1)
    w = engine.mx_quantize({"k": x.to(DEV)}, fmt)
    same(f"boundaries/{fmt}", w["k"], w.scales["k"], x, fmt)


@oracle
@pytest.mark.parametrize("layout", ["off_4_bytes", "strided", "pinned_host"])
@pytest.mark.parametrize("fmt", FMTS)
def test_layouts(fmt, layout):
    from flame_amd import engine
    x = _key(CHUNK + 300, torch.Generator().manual_seed(5), torch.float32)
    src = {"off_4_bytes": lambda: torch.empty(x.numel() + 1, device=DEV)[1:].copy_(x),
           "strided": lambda: torch.stack([x, x + 1], dim=1).to(DEV)[:, 0],
           "pinned_host": lambda: x.clone().pin_memory()}[layout]()
    w = engine.mx_quantize({"k": src}, fmt, device=DEV)
    same(f"{layout}/{fmt}", w["k"], w.scales["k"], x, fmt)


@oracle
@pytest.mark.parametrize("fmt", FMTS)
def test_through_the_encoder(fmt):
    import cloudpickle
    from flame_amd import egress, mx
    g = torch.Generator().manual_seed(9)
    model = OrderedDict([("w", _key(33 * 43, g, torch.float32).view(33, 43)), ("b", torch.randn(40, generator=g)),
                         ("steps", torch.tensor([7, 9], dtype=torch.int64))])
    weights = OrderedDict((k, v.to(DEV)) for k, v in model.items())
    msg = {"weights": weights, "round": 3, "meta": {"n": 5}}
    got = cloudpickle.loads(egress.MessageEncoder(mx=fmt, mx_min_numel=64).encode_bytes(msg))
    consult.note()
    ref = mx.quantize(model, fmt, 64)
    assert isinstance(got["weights"], mx.MXWeights) and got["round"] == 3 and got["meta"] == {"n": 5}
    assert list(got["weights"].scales) == ["w"] and torch.equal(got["weights"].scales["w"], ref.scales["w"])
    a, b = mx.dequantize(got["weights"]), mx.dequantize(ref)
    assert a["w"].shape == (33, 43) and torch.equal(a["w"].view(torch.int32)[~b["w"].isnan()], b["w"].view(torch.int32)[~b["w"].isnan()])
    assert torch.equal(a["w"].isnan(), b["w"].isnan()) and torch.equal(a["b"], model["b"]) and torch.equal(a["steps"], model["steps"])
    assert msg["weights"] is weights and all(weights[k].dtype == model[k].dtype for k in model)
    with Launches() as ln:              # mx=None: the parent's payload, and no quantiser launch
        plain = pickle.loads(egress.MessageEncoder().encode_bytes(msg))
    assert ln.names == [] and all(torch.equal(plain["weights"][k].view(torch.uint8), model[k].view(torch.uint8)) for k in model)
    assert len(egress.MessageEncoder(mx=None).encode(msg)) == len(egress.MessageEncoder().encode(msg))


def test_late_stream():
    from flame_amd import engine
    x = _key(3 * CHUNK + 5, torch.Generator().manual_seed(3), torch.float32)
    delay = SC.Delay()

    def case(late):
        src = late.tensor(x)
        with late.stream():
            late.start()
            with late.call("mx_quantize"):
                w = engine.mx_quantize({"k": src}, "e2m1")
            res = late.snap({"q": w["k"].view(torch.uint8), "s": w.scales["k"]})
        late.finish()
        return {"mx": SC.cpu(res)}
    ready = case(SC.Late(delay, ready=True))
    late_res = case(SC.Late(delay))
    delay.free()
    SC.assert_same("mx_quantize", ready, late_res)
    same("late", late_res["mx"]["q"], late_res["mx"]["s"], x, "e2m1")
