"""GPU: the sign packer (flame_onebit_pack, engine.sign_pack_ / engine.sign_compress, MessageEncoder(sign=True)) against
flame_amd.sign's torch statements on the CPU, by the contract of DESIGN.md §2.  Everything is compared bit for bit."""
from collections import OrderedDict

import pytest
import torch

import stream_case as SC
from flame_amd import _native as N
from flame_amd import egress, engine, sign
from flame_amd.optimizers import optimizer_provider
from large_case import Launches
from test_mx_host import _cache

pytestmark = [pytest.mark.gpu]
DEV, WHO = "cuda:0", "flame_onebit_pack"
SRCS = [torch.float32, torch.bfloat16, torch.float16]


def _key(n, g, dtype=torch.float32):
    """``n`` values, every run of 32 at its own power-of-two magnitude, some zeros, -0 and subnormals, +-inf; no NaN."""
    mag = torch.exp2(torch.randint(-30, 13, (-(-n // 32),), generator=g).float()).repeat_interleave(32)[:n]
    x = torch.randn(n, generator=g) * mag
    x[torch.rand(n, generator=g) < 0.03] = 0.0
    x[torch.rand(n, generator=g) < 0.02] = -0.0
    x[torch.rand(n, generator=g) < 0.02], x[torch.rand(n, generator=g) < 0.02] = 1e-41, -3e-42
    if n > 200:
        x[70], x[101] = float("inf"), float("-inf")
    return x.to(dtype)


def same(label, bits, scales, d):
    """``bits`` / ``scales`` are those of the fp32 CPU tensor ``d``: signbit packed by sign.compress_tensor, scales in the fold order."""
    want = sign.compress_tensor(d, fold=True)
    assert bits.dtype == torch.uint8 and torch.equal(bits.cpu(), want[0]), f"{label}: bits differ"
    assert scales.dtype == torch.float32 and torch.equal(scales.cpu().view(torch.int32), want[1].view(torch.int32)), f"{label}: scales differ"
    return want


@pytest.mark.parametrize("src", SRCS, ids=str)
def test_shapes_and_extents(src):
    """Every numel as one segment of ONE call, guard elements behind every output."""
    C = int(N.lib().flame_onebit_pack_chunk_elems())
    numels = [1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 37]
    g = torch.Generator().manual_seed(21)
    xs = [_key(n, g, src) for n in numels]
    nw, nb = [8 * -(-n // 64) for n in numels], [-(-n // 256) for n in numels]
    bits, scales = [torch.full((w + 16,), 0xA5, dtype=torch.uint8, device=DEV) for w in nw], [torch.full((b + 16,), -7.0, device=DEV) for b in nb]
    with Launches() as ln:
        engine.sign_pack_([x.to(DEV) for x in xs], [t[:w] for t, w in zip(bits, nw)], [t[:b] for t, b in zip(scales, nb)])
    torch.cuda.synchronize()
    assert ln.names == [WHO], ln.names
    for n, x, t, w, s, b in zip(numels, xs, bits, nw, scales, nb):
        same(f"{src}/n={n}", t[:w], s[:b], x.float())
        assert bool((t[w:] == 0xA5).all()) and bool((s[b:] == -7.0).all()), f"n={n}: written past the extent"


@pytest.mark.parametrize("layout", ["aligned", "off_4_bytes", "strided", "pinned_host"])
def test_base(layout):
    g = torch.Generator().manual_seed(6)
    n = int(N.lib().flame_onebit_pack_chunk_elems()) + 300
    x, b = _key(n, g), torch.randn(n, generator=g)
    b[::3] = x[::3]                                              # a third of the changes are zeros
    off = layout == "off_4_bytes"
    src = {"aligned": lambda: x.to(DEV), "off_4_bytes": lambda: torch.empty(n + 1, device=DEV)[1:].copy_(x),
           "strided": lambda: torch.stack([x, x + 1], dim=1).to(DEV)[:, 0], "pinned_host": lambda: x.clone().pin_memory()}[layout]()
    shaped = layout in ("aligned", "pinned_host")
    runs = []
    for _ in range(2):                                           # the same call from the same state: the same bytes
        base = (torch.empty(n + 1, device=DEV)[1:] if off else torch.empty(n, device=DEV)).copy_(b)
        with Launches() as ln:
            w = engine.sign_compress({"k": src.view(4, -1) if shaped else src}, base={"k": base}, device=DEV)
        assert ln.names == [WHO] and w.shapes["k"] == ((4, n // 4) if shaped else (n,))
        runs.append((w["k"].cpu(), w.scales["k"].cpu().view(torch.int32), base.cpu().view(torch.int32)))
    assert all(torch.equal(p, q) for p, q in zip(*runs)), "two equal calls differ"
    rb, rs = same(layout, w["k"], w.scales["k"], x - b)
    assert torch.equal(runs[0][2], (b + sign.dequantize_tensor(rb, rs, (n,))).view(torch.int32)), "the base is not f32(base + sent)"
    with pytest.raises(TypeError):
        engine.sign_compress({"k": x.to(DEV).half()}, base={"k": base})


def test_through_the_encoder():
    import cloudpickle
    g = torch.Generator().manual_seed(9)
    finite = lambda t: t.nan_to_num(0.0, 3.0, -3.0)             # noqa: E731
    model = OrderedDict([("w", finite(_key(33 * 43, g)).view(33, 43)), ("b", torch.randn(40, generator=g)),
                         ("steps", torch.tensor([7, 9], dtype=torch.int64))])
    enc, trainer, ref = egress.MessageEncoder(sign=True, sign_min_numel=64), OrderedDict(), None
    for rnd in range(6):
        if rnd:
            model["w"] = model["w"] + finite(_key(33 * 43, g)).view(33, 43) * 0.01
            model["b"], model["steps"] = model["b"] + 1, model["steps"] + 1
        if rnd == 4:
            enc.reset()
        msg = {"weights": OrderedDict((key, v.to(DEV)) for key, v in model.items()), "round": rnd}
        got = cloudpickle.loads(enc.encode_bytes(msg))
        dense = rnd in (0, 4)
        assert isinstance(got["weights"], sign.SignWeights) != dense and got["round"] == rnd
        if dense:
            ref = model["w"].clone()
        else:
            assert list(got["weights"].scales) == ["w"] and got["weights"].shapes["w"] == (33, 43)
            rb, rs = same(f"round {rnd}", got["weights"]["w"], got["weights"].scales["w"], model["w"] - ref)
            ref = ref + sign.dequantize_tensor(rb, rs, (33, 43))
        sign.apply_(trainer, got["weights"])
        assert torch.equal(trainer["w"].view(torch.int32), ref.view(torch.int32)), f"round {rnd}: the trainer left the base"
        assert torch.equal(enc._base["w"].cpu().view(torch.int32), ref.view(torch.int32)) and list(enc._base) == ["w"]
        assert torch.equal(trainer["b"], model["b"]) and torch.equal(trainer["steps"], model["steps"])
        assert torch.equal(msg["weights"]["w"].cpu(), model["w"])       # the caller's tensors are untouched
    with Launches() as ln:              # sign=False: the parent's payload, and no launch
        plain = len(egress.MessageEncoder(sign=False).encode(msg))
    assert ln.names == [] and plain == len(egress.MessageEncoder().encode(msg))
    # the uplink closes the loop
    ups = [engine.sign_compress({"w": torch.randn(33, 43, generator=g).to(DEV)}) for _ in range(2)]
    outs = [optimizer_provider.get("fedavg").do({"w": model["w"].to(DEV)}, _cache(ws, [2, 3]), total=5)
            for ws in (ups, [{"w": sign.dequantize(u)["w"]} for u in ups])]
    assert torch.equal(outs[0]["w"].view(torch.int32), outs[1]["w"].view(torch.int32)) and not torch.equal(outs[0]["w"].cpu(), model["w"])


def test_late_stream():
    x = _key(3 * int(N.lib().flame_onebit_pack_chunk_elems()) + 5, torch.Generator().manual_seed(3))
    delay = SC.Delay()

    def case(late):
        src = late.tensor(x)
        with late.stream():
            late.start()
            with late.call("sign_compress"):
                w = engine.sign_compress({"k": src})
            res = late.snap({"b": w["k"], "s": w.scales["k"].view(torch.int32)})
        late.finish()
        return {"pack": SC.cpu(res)}
    ready, late_res = case(SC.Late(delay, ready=True)), case(SC.Late(delay))
    delay.free()
    SC.assert_same("pack", ready, late_res)
    same("late", late_res["pack"]["b"], late_res["pack"]["s"].view(torch.float32), x)
