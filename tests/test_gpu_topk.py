"""GPU: the top-k selection (flame_topk_select, engine.topk_ / engine.topk, MessageEncoder(sparse=)) against
tests/topk_ref.py, by the contract of DESIGN.md §2.  Everything is compared bit for bit."""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import stream_case as SC
import topk_ref as R
from large_case import Launches

pytestmark = [pytest.mark.gpu]
DEV, WHO, C = "cuda:0", "flame_topk_select", 4096
SRCS = [torch.float32, torch.bfloat16, torch.float16]
NUMELS = [1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 37]
KS = {"one": lambda n: 1, "1pct": lambda n: math.ceil(0.01 * n), "half": lambda n: max(1, n // 2), "all": lambda n: n}


def _key(n, g, dtype=torch.float32):
    """``n`` values, every run of 32 at its own magnitude, some zeros and -0, one NaN, +-inf."""
    mag = torch.exp2(torch.randint(-30, 13, (-(-n // 32),), generator=g).float()).repeat_interleave(32)[:n]
    x = torch.randn(n, generator=g) * mag
    x[torch.rand(n, generator=g) < 0.03] = 0.0
    x[torch.rand(n, generator=g) < 0.02] = -0.0
    if n > 200:
        x[37], x[70], x[101] = float("nan"), float("inf"), float("-inf")
    return x.to(dtype)


def same(label, idx, val, x, k, base=None, f16=False):
    """``idx`` / ``val`` are the reference's selection of the fp32 array ``x``; returns the reference's base.
    ``f16``: an f16 NaN comes out as some NaN.  With a base a NaN difference is some NaN too (IEEE 754 leaves
    the payload a subtract propagates to the implementation)."""
    ri, rv, rb = R.topk(x, k, base)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert idx.dtype == np.int32 and val.dtype == np.float32 and idx.shape == val.shape == (k,), label
    assert np.array_equal(idx, ri), f"{label}: indices differ, first at {np.flatnonzero(idx != ri)[:1]}"
    nan = np.isnan(rv) if f16 or base is not None else np.zeros(k, dtype=bool)
    assert np.array_equal(val.view(np.uint32)[~nan], rv.view(np.uint32)[~nan]) and np.isnan(val[nan]).all(), f"{label}: values differ"
    return rb


def select(x, k):
    """One ``topk_`` call over the 1-D tensor ``x``: (indices, values) on the device."""
    from flame_amd import engine
    val, idx = torch.empty(k, device=DEV), torch.empty(k, dtype=torch.int32, device=DEV)
    engine.topk_([x.to(DEV)], [val], [idx], [k])
    return idx, val


@pytest.mark.parametrize("src", SRCS, ids=str)
@pytest.mark.parametrize("kind", list(KS))
def test_shapes_and_extents(kind, src):
    """Every numel as one segment of ONE call, guard elements behind every output."""
    from flame_amd import engine
    g = torch.Generator().manual_seed(21)
    xs = [_key(n, g, src) for n in NUMELS]
    ks = [KS[kind](n) for n in NUMELS]
    vals = [torch.full((k + 16,), -7.0, device=DEV) for k in ks]
    idxs = [torch.full((k + 16,), -7, dtype=torch.int32, device=DEV) for k in ks]
    with Launches() as ln:
        engine.topk_([x.to(DEV) for x in xs], [v[:k] for v, k in zip(vals, ks)], [i[:k] for i, k in zip(idxs, ks)], ks)
    torch.cuda.synchronize()
    assert ln.names == [WHO], ln.names
    for n, x, k, v, i in zip(NUMELS, xs, ks, vals, idxs):
        same(f"{kind}/{src}/n={n}", i[:k], v[:k], R.f32(x), k, f16=src == torch.float16)
        assert bool((v[k:] == -7.0).all()) and bool((i[k:] == -7).all()), f"n={n}: written past the extent"


def _tie_case(name, n, g):
    """(fp32 tensor, k) of the ties-and-digits cases."""
    bits = lambda b: b.to(torch.int32).view(torch.float32)     # noqa: E731
    if name == "classes":           # the threshold is the 1 class; fewer ties are wanted than there are
        x = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0, float("nan")])[torch.randint(0, 6, (n,), generator=g)]
        above = int((x.abs() > 1).sum() + x.isnan().sum())
        return x, above + int((x.abs() == 1).sum()) // 2
    if name == "all_equal":
        return torch.full((n,), -1.5), n // 3
    if name == "subnormals":        # subnormals against zeros: every subnormal and three of the zeros
        x = bits(torch.randint(0, 4, (n,), generator=g) * torch.randint(0, 2, (n,), generator=g)) * torch.tensor([1.0, -1.0])[torch.randint(0, 2, (n,), generator=g)]
        return x, int((x != 0).sum()) + 3
    lo, width = {"digit_lo": (0, 9), "digit_mid": (9, 11), "digit_hi": (20, 11)}[name]
    field = torch.randint(0, 1 << width, (n,), generator=g) << lo
    return bits(field | (0 if name == "digit_hi" else 0x3F800000)), n // 7


@pytest.mark.parametrize("name", ["classes", "all_equal", "subnormals", "digit_lo", "digit_mid", "digit_hi"])
def test_ties_and_digits(name):
    x, k = _tie_case(name, 3 * C + 5, torch.Generator().manual_seed(4))
    same(name, *select(x, k), R.f32(x), k)


def test_many_chunks():
    """More chunks than one step of the scan workgroup covers (256)."""
    n = 257 * C + 11
    x = torch.randn(n, generator=torch.Generator().manual_seed(8))
    k = math.ceil(0.01 * n)
    same("many chunks", *select(x, k), R.f32(x), k)


@pytest.mark.parametrize("layout", ["aligned", "off_4_bytes", "strided", "pinned_host"])
def test_base(layout):
    from flame_amd import engine
    g = torch.Generator().manual_seed(6)
    n = C + 300
    x, b = _key(n, g), torch.randn(n, generator=g)
    b[::3] = x[::3]                                              # a third of the changes are zeros
    off = layout == "off_4_bytes"
    src = {"aligned": lambda: x.to(DEV), "off_4_bytes": lambda: torch.empty(n + 1, device=DEV)[1:].copy_(x),
           "strided": lambda: torch.stack([x, x + 1], dim=1).to(DEV)[:, 0], "pinned_host": lambda: x.clone().pin_memory()}[layout]()
    base = (torch.empty(n + 1, device=DEV)[1:] if off else torch.empty(n, device=DEV)).copy_(b)
    with Launches() as ln:
        w = engine.topk({"k": src.view(4, -1) if layout in ("aligned", "pinned_host") else src}, 0.05, base={"k": base}, device=DEV)
    assert ln.names == [WHO] and w.shapes["k"] == ((4, n // 4) if layout in ("aligned", "pinned_host") else (n,))
    rb = same(layout, w.indices["k"], w["k"], R.f32(x), math.ceil(0.05 * n), base=R.f32(b))
    ok = ~np.isnan(rb)
    assert np.array_equal(R.f32(base).view(np.uint32)[ok], rb.view(np.uint32)[ok]) and np.isnan(R.f32(base)[~ok]).all(), \
        "the base is not f32(base + d) where sent, untouched elsewhere"
    with pytest.raises(TypeError):
        engine.topk({"k": x.to(DEV).half()}, 0.05, base={"k": base})


def test_through_the_encoder():
    import cloudpickle
    from flame_amd import egress, sparse
    g = torch.Generator().manual_seed(9)
    finite = lambda t: t.nan_to_num(0.0, 3.0, -3.0)             # noqa: E731  (a NaN change has no stated payload)
    model = OrderedDict([("w", finite(_key(33 * 43, g)).view(33, 43)), ("b", torch.randn(40, generator=g)),
                         ("steps", torch.tensor([7, 9], dtype=torch.int64))])
    enc, trainer, ref = egress.MessageEncoder(sparse=0.1, sparse_min_numel=64), OrderedDict(), None
    k = math.ceil(0.1 * 33 * 43)
    for rnd in range(6):
        if rnd:
            model["w"] = model["w"] + finite(_key(33 * 43, g)).view(33, 43) * 0.01
            model["b"], model["steps"] = model["b"] + 1, model["steps"] + 1
        if rnd == 4:
            enc.reset()
        msg = {"weights": OrderedDict((key, v.to(DEV)) for key, v in model.items()), "round": rnd}
        got = cloudpickle.loads(enc.encode_bytes(msg))
        dense = rnd in (0, 4)
        assert isinstance(got["weights"], sparse.SparseWeights) != dense and got["round"] == rnd
        if dense:
            ref = R.f32(model["w"])
        else:
            assert list(got["weights"].indices) == ["w"] and got["weights"].shapes["w"] == (33, 43)
            ref = same(f"round {rnd}", got["weights"].indices["w"], got["weights"]["w"], R.f32(model["w"]), k, base=ref)
        sparse.apply_(trainer, got["weights"])
        assert np.array_equal(R.f32(trainer["w"]).view(np.uint32), ref.view(np.uint32)), f"round {rnd}: the trainer left the base"
        assert np.array_equal(R.f32(enc._base["w"]).view(np.uint32), ref.view(np.uint32)) and list(enc._base) == ["w"]
        assert torch.equal(trainer["b"], model["b"]) and torch.equal(trainer["steps"], model["steps"])
        assert torch.equal(msg["weights"]["w"].cpu(), model["w"])       # the caller's tensors are untouched (all finite)
    with Launches() as ln:              # sparse=None: the parent's payload, and no launch
        plain = len(egress.MessageEncoder(sparse=None).encode(msg))
    assert ln.names == [] and plain == len(egress.MessageEncoder().encode(msg))


def test_late_stream():
    from flame_amd import engine
    x = _key(3 * C + 5, torch.Generator().manual_seed(3))
    delay = SC.Delay()

    def case(late):
        src = late.tensor(x)
        with late.stream():
            late.start()
            with late.call("topk"):
                w = engine.topk({"k": src}, 0.01)
            res = late.snap({"i": w.indices["k"], "v": w["k"].view(torch.int32)})
        late.finish()
        return {"topk": SC.cpu(res)}
    ready = case(SC.Late(delay, ready=True))
    late_res = case(SC.Late(delay))
    delay.free()
    SC.assert_same("topk", ready, late_res)
    same("late", late_res["topk"]["i"], late_res["topk"]["v"].view(torch.float32), R.f32(x), math.ceil(0.01 * x.numel()))
