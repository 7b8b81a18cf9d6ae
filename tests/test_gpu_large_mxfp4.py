"""flame_agg_reduce_mxfp4 on a key whose element index crosses 2^32 (tests/large_case.py:
``P16 = 2^32 + 70,001``), as tests/test_gpu_large_kernels.py has it for flame_agg_reduce_mx: an element
index, its byte index e >> 1 and its scale index e / 32 evaluated in 32 bits would wrap.  Sampled
bitwise at ``large_case.index(P16)``; the part at or past 2^32 is also read by a contiguous slice."""
import pytest
import torch

import large_case as LC
import scenarios as S
import uplink16_case as U
from large_case import DEV, P16, Launches, _at, _free, _need

pytestmark = [pytest.mark.gpu]


def _bytes_at(t, i, past):
    """``t`` (uint8, on the device) at the indices ``i`` by index_select -- and, where the ELEMENT index is
    at or past 2^32 (``past``), by a contiguous slice as well: these inputs have no host restatement, so
    the sampler itself is checked where a wrapped sampler would make the comparison vacuous."""
    got = _at(t, i)
    lo = int(i[past].min())
    assert torch.equal(got[past], t[lo:].cpu()[i[past] - lo])
    return got


def test_reduce_mxfp4_past_2_32_elements():
    """Two MXFP4 clients of random packed bytes and scale bytes 2^-8 .. 2^8 into an fp32 aggregate; element
    e is nibble e & 1 of byte e >> 1, its scale byte is at e / 32."""
    from flame_amd import engine, mx
    nbytes, nb = (P16 + 1) // 2, mx.n_blocks(P16)
    _need(4 * P16 / 1e9 + 2 * nbytes / 1e9 + 2 * nb / 1e9 + 3)      # the fp32 base, two packed clients, their scales
    idx = LC.index(P16)
    past = idx >= 1 << 32
    assert int(past.sum()) == P16 - (1 << 32)
    seed = LC.SEED["mx"]
    b_s = LC.host_synth(seed, 0, idx, 1.0)
    base = LC._synth(P16, seed, 0, 1.0)
    LC.pinned("mxfp4 base", base, idx, b_s)
    g = torch.Generator(device=DEV).manual_seed(seed + 4)
    qs = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=DEV, generator=g) for _ in range(2)]
    ss = [torch.randint(119, 136, (nb,), dtype=torch.uint8, device=DEV, generator=g) for _ in range(2)]
    deq = []
    for q, s in zip(qs, ss):
        # mx.dequantize over blocks that hold the sample in their first element (the low nibble of byte 0)
        code = (_bytes_at(q, idx >> 1, past) >> (4 * (idx & 1)).to(torch.uint8)) & 15
        blocks = torch.zeros(idx.numel(), mx.BLOCK // 2, dtype=torch.uint8)
        blocks[:, 0] = code
        w = mx.MXWeights({"w": blocks.view(-1).view(mx.PACKED)}, {"w": _bytes_at(s, idx // mx.BLOCK, past)},
                         shapes={"w": (idx.numel() * mx.BLOCK,)})
        deq.append(mx.dequantize(w)["w"][::mx.BLOCK].contiguous())
    ws = [mx.MXWeights({"w": q.view(mx.PACKED)}, {"w": s}, shapes={"w": (P16,)}) for q, s in zip(qs, ss)]
    with Launches() as ln:
        engine.accumulate({"w": base}, list(zip(ws, LC.RATES)))
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_mxfp4"], ln.names
    S.same_bits("mxfp4", {"w": _at(base, idx)}, {"w": U.restate(b_s, deq, LC.RATES)})
    del base, qs, ss, ws
    _free()
