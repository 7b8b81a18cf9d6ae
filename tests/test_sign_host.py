"""flame_amd.sign on the host: the format at its edges, pickling, error feedback; engine.sign_route's refusals, engine.plan_sign's table."""
import pickle

import numpy as np
import pytest
import torch

from flame_amd import engine, lowrank, mx, sign, sparse


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("numel", [1, 63, 64, 65, 255, 256, 257, 515])
def test_compress_and_dequantize(numel, dtype):
    """Bit e is signbit(x[e]) (-0.0 gives 1), pad bits are 0, a scale is the block's fp32 mean magnitude (an all-zero block: 0);
    int keys and keys under min_numel pass through."""
    x = (torch.arange(numel, dtype=torch.float32) % 7 - 3).to(dtype)
    x[0], x[256:512] = -0.0, 0.0
    w = sign.compress({"x": x, "n": torch.tensor(3)})
    assert list(w.scales) == ["x"] and w.shapes == {"x": (numel,)} and not sign.compress({"x": x}, min_numel=numel + 1).scales
    assert w["x"].dtype == torch.uint8 and w["x"].shape == (8 * -(-numel // 64),) and w.scales["x"].dtype == torch.float32
    bits = np.unpackbits(w["x"].numpy(), bitorder="little")
    assert np.array_equal(bits[:numel], torch.signbit(x).numpy()) and bits[0] == 1 and not bits[numel:].any()
    want = [np.float32(x.float().numpy()[b:b + 256].__abs__().sum(dtype=np.float32) / np.float32(min(256, numel - b))) for b in range(0, numel, 256)]
    assert np.array_equal(w.scales["x"].numpy(), np.array(want, dtype=np.float32)) and (numel <= 256 or w.scales["x"][1] == 0)
    d = sign.dequantize(w)
    assert d["x"].dtype == torch.float32 and d["x"].shape == x.shape and torch.equal(torch.signbit(d["x"]), torch.signbit(x))
    assert torch.equal(d["x"].abs(), w.scales["x"].repeat_interleave(256)[:numel]) and d["n"] is w["n"]
    r = pickle.loads(pickle.dumps(w))       # the round trip keeps the class, the order and all three parts
    assert type(r) is sign.SignWeights and r.shapes == w.shapes and list(r) == ["x", "n"] and torch.equal(r["n"], w["n"])
    assert torch.equal(r["x"], w["x"]) and torch.equal(r.scales["x"], w.scales["x"])


def test_error_feedback():
    """Multiples of 1/8 below 4 over whole blocks: every scale, sum and difference is exact, so sent + residual IS delta + old residual."""
    g = torch.Generator().manual_seed(5)
    ef, deltas = sign.ErrorFeedback(), [{"x": torch.randint(-16, 17, (2, 256), generator=g) / 8, "n": torch.tensor(1)} for _ in range(2)]
    first = ef.compress(deltas[0])
    old = ef.residual["x"].clone()
    assert torch.equal(sign.dequantize(first)["x"] + old, deltas[0]["x"]) and list(ef.residual) == ["x"] and bool(old.any())
    second = ef.compress(deltas[1])
    assert torch.equal(sign.dequantize(second)["x"] + ef.residual["x"], deltas[1]["x"] + old)
    ef.reset()
    assert ef.residual == {} and torch.equal(ef.compress(deltas[0])["x"], first["x"])


_GOOD = sign.compress({"w": torch.ones(300)})
_with = lambda bits=None, scales=None, shapes=None: sign.SignWeights(      # noqa: E731
    {"w": _GOOD["w"] if bits is None else bits}, {"w": _GOOD.scales["w"] if scales is None else scales}, _GOOD.shapes if shapes is None else shapes)
ROUTE_REFUSED = {
    "dense": {"w": torch.ones(300)}, "mx": mx.quantize({"w": torch.ones(300)}), "sparse": sparse.topk({"w": torch.ones(300)}),
    "lowrank": lowrank.LowRankWeights({"w": torch.ones(300, 1)}, {"w": torch.ones(1, 1)}, {"w": (300,)}),
    "bf16_aggregate": torch.bfloat16, "f16_aggregate": torch.float16,
    "bits_dtype": _with(bits=_GOOD["w"].to(torch.int8)), "bits_dim": _with(bits=_GOOD["w"].view(5, 8)), "bits_count": _with(bits=_GOOD["w"][:-8]),
    "scales_dtype": _with(scales=_GOOD.scales["w"].double()), "scales_dim": _with(scales=_GOOD.scales["w"].view(2, 1)),
    "scales_count": _with(scales=_GOOD.scales["w"][:1]), "no_shape": _with(shapes={}), "wrong_shape": _with(shapes={"w": (301,)}),
}


@pytest.mark.parametrize("what", list(ROUTE_REFUSED))
def test_sign_route_refuses(what):
    bad = ROUTE_REFUSED[what]
    assert engine.sign_route(torch.float32, [_GOOD, _GOOD], "w", (300,)) is True and engine.sign_route(torch.float32, [{"w": 1}], "w", (300,)) is False
    with pytest.raises(TypeError, match="(?i)sign update.*supported"):
        if isinstance(bad, torch.dtype):
            engine.sign_route(bad, [_GOOD, _GOOD], "w", (300,))
        else:
            engine.sign_route(torch.float32, [_GOOD, bad], "w", (300,))


def test_plan_sign():
    """Keys of 16,385 and 5 elements over three clients, then the ragged group: one key of 0 and one of 16,384 over two."""
    segs = [engine.Seg(16385, out=4096, inp=8192), engine.Seg(5, out=12288, inp=12288)]
    meta, n_chunks, o = engine.plan_sign(segs, [[8, 16, 24], [32, 40, 48]], [[4, 12, 20], [28, 36, 44]], [0.5, 0.25, 0.1], chunk=16384)
    assert n_chunks == 3 and o == {"segs": 0, "bits": 160, "scales": 208, "r32": 256} and meta.nbytes == 272
    head = meta[:20].reshape(2, 10)
    assert head[0].tolist() == [4096, 8192, 0, 0, 0, 0, 16385, 0, 0, 0] and head[1].tolist() == [12288, 12288, 0, 0, 0, 0, 5, 2, 0, 0]
    assert meta[20:26].tolist() == [8, 16, 24, 32, 40, 48] and meta[26:32].tolist() == [4, 12, 20, 28, 36, 44]
    assert meta[32:].view(np.float32).tolist() == [0.5, 0.25, np.float32(0.1), 0.0]
    meta, n_chunks, o = engine.plan_sign([engine.Seg(0), engine.Seg(16384, out=64, inp=64)], [[0, 0], [8, 16]], [[0, 0], [4, 4]], [1.0, 2.0], chunk=16384)
    assert n_chunks == 1 and meta[:20].reshape(2, 10)[:, 6:8].tolist() == [[0, 0], [16384, 0]] and o["r32"] == 224 and meta.nbytes == 232
