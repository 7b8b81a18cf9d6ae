"""flame_mx_quantize past 2^32 elements (tests/large_case.py: ``P16 = 2^32 + 70,001``), where e, e >> 1 and e / 32
would wrap in 32 bits: the whole source blocks around ``large_case.index(P16)``, quantised on the CPU, against
the nibbles and scale bytes there."""
import pytest
import torch

import large_case as LC
from large_case import DEV, P16, Launches, _at, _free, _need

pytestmark = [pytest.mark.gpu]


def _bytes_at(t, i, past):
    """``t`` at ``i`` by index_select, and where ``past`` by a contiguous slice as well: the sampler is checked too."""
    got = _at(t, i)
    lo = int(i[past].min())
    assert torch.equal(got[past], t[lo:].cpu()[i[past] - lo])
    return got


def test_mx_quantize_past_2_32_elements():
    from flame_amd import engine, mx
    _need(2 * P16 / 1e9 + P16 / 2e9 + P16 / 32e9 + 3)       # a bf16 source, its nibbles and scale bytes
    blk = torch.unique(LC.index(P16) // mx.BLOCK)
    blk = blk[blk < P16 // mx.BLOCK]                         # whole blocks (the ragged last one: test_gpu_mx_quantize.py)
    past = blk >= (1 << 32) // mx.BLOCK
    assert int(past.sum()) == (P16 - (1 << 32)) // mx.BLOCK
    elems = (blk.view(-1, 1) * mx.BLOCK + torch.arange(mx.BLOCK)).view(-1)
    src = LC._synth(P16, LC.SEED["mx"], 0, 1.0, torch.bfloat16)
    x = LC.pinned("mx_quantize source", src, elems, LC.host_synth(LC.SEED["mx"], 0, elems, 1.0, torch.bfloat16))
    with Launches() as ln:
        w = engine.mx_quantize({"w": src}, "e2m1")
    torch.cuda.synchronize()
    assert ln.names == ["flame_mx_quantize"], ln.names
    ref = mx.quantize({"w": x}, "e2m1")
    byte = (blk.view(-1, 1) * (mx.BLOCK // 2) + torch.arange(mx.BLOCK // 2)).view(-1)
    assert torch.equal(_bytes_at(w["w"].view(torch.uint8), byte, byte >= 1 << 31), ref["w"].view(torch.uint8))
    assert torch.equal(_bytes_at(w.scales["w"], blk, past), ref.scales["w"])
    del src, w
    _free()
