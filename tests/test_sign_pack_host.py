"""The sign packer's host side: sign.fold_scales (the definition of the device's scales), compress(fold=True), sign.apply_,
engine.plan_sign_pack, flame_onebit_pack's refusals and the encoder's.  No GPU call."""
import ctypes

import numpy as np
import pytest
import torch

from flame_amd import _native as N
from flame_amd import egress, engine, sign


@pytest.mark.parametrize("numel", [1, 255, 256, 257, 515])
def test_fold_scales_against_fp64(numel):
    """Eight nonnegative fp32 adds and one division: at most (1 + 2^-24)^9 - 1 < 10 * 2^-24 from the fp64 mean magnitude."""
    x = torch.randn(numel, generator=torch.Generator().manual_seed(numel)) * 3
    want = np.array([np.abs(x.double().numpy()[b:b + 256]).sum() / min(256, numel - b) for b in range(0, numel, 256)])
    got = sign.fold_scales(x)
    assert got.dtype == torch.float32 and got.shape == (len(want),) and (np.abs(got.double().numpy() - want) <= 10 * 2.0 ** -24 * want).all()
    ints = torch.arange(numel, dtype=torch.float32) % 7 - 3            # small integers: every order of the sum is exact
    assert torch.equal(sign.fold_scales(ints), sign.compress_tensor(ints)[1])


def test_compress_fold():
    g = torch.Generator().manual_seed(1)
    w = {"x": torch.randn(3, 300, generator=g), "h": torch.randn(70, generator=g).bfloat16(), "n": torch.tensor(3)}
    a, b = sign.compress(w, min_numel=64), sign.compress(w, min_numel=64, fold=True)
    assert list(b.scales) == ["x", "h"] and b.shapes == a.shapes and b["n"] is w["n"]
    for k in b.scales:
        assert torch.equal(a[k], b[k]) and torch.equal(b.scales[k], sign.fold_scales(w[k]))


def test_apply():
    """Two messages: the compressed key is base0 + deq(m1) + deq(m2) in that order; every other key is copied."""
    g = torch.Generator().manual_seed(2)
    base0 = torch.randn(5, 77, generator=g)
    model = {"w": base0.clone(), "b": torch.zeros(3), "n": torch.tensor(1)}
    msgs = [sign.compress({"w": torch.randn(5, 77, generator=g), "b": torch.full((3,), float(i)), "n": torch.tensor(i)}, min_numel=64, fold=True)
            for i in (4, 5)]
    want = base0
    for m in msgs:
        assert sign.apply_(model, m) is model
        want = want + sign.dequantize(m)["w"]
    assert torch.equal(model["w"], want) and torch.equal(model["b"], torch.full((3,), 5.0)) and model["n"] == 5


def test_plan_sign_pack():
    C = 512
    segs = [engine.Seg(0, out=8, inp=4, cur_out=4), engine.Seg(5, out=0x1000, inp=0x2004, cur_out=0x3000, m=0x4004),
            engine.Seg(C + 1, out=0x5000, inp=0x6000, cur_out=0x7000)]
    meta, n_chunks = engine.plan_sign_pack(segs, chunk=C)
    head = meta.reshape(3, engine.SEG_WORDS)
    assert n_chunks == 3 and head[:, 6].tolist() == [0, 5, C + 1] and head[:, 7].tolist() == [0, 0, 1]
    assert head[1].tolist() == [0x1000, 0x2004, 0, 0x3000, 0x4004, 0, 5, 0, 0, 0]       # out, in, -, cur_out, m
    with pytest.raises(ValueError, match="8-byte"):
        engine.plan_sign_pack([engine.Seg(5, out=0x1004, inp=0x2000, cur_out=0x3000)], chunk=C)


def test_entry_point_refusals():
    L, FAKE, err = N.lib(), ctypes.c_void_p(4096), N.lib().flame_last_error     # FAKE is never dereferenced: every call fails on the host
    assert L.flame_onebit_pack_chunk_elems() == 4096 and L.flame_launch_branches() == 100 and L.flame_abi_version() == 1
    args = {"sd": N.FLAME_F32, "flags": 0, "segs": FAKE, "n_segs": 1, "n_chunks": 2}
    call = lambda **kw: L.flame_onebit_pack(*{**args, **kw}.values(), None)      # noqa: E731
    for k, v, text in [("segs", None, b"segment"), ("segs", ctypes.c_void_p(4100), b"8-byte aligned"), ("n_segs", 0, b"segment"),
                       ("n_chunks", 0, b"n_chunks"), ("n_chunks", 2 ** 31, b"n_chunks"), ("flags", 2, b"unknown flags"),
                       ("flags", 1 << 20, b"unknown flags")]:
        assert call(**{k: v}) == N.FLAME_EINVAL and b"flame_onebit_pack" in err() and text in err(), (k, err())
    for sd in (N.FLAME_F64, N.FLAME_I32, N.FLAME_FP4_E2M1, 13, -1):
        assert call(sd=sd) == N.FLAME_ENOTSUP and b"flame_onebit_pack" in err() and b"source dtype %d" % sd in err()
    for sd in (N.FLAME_BF16, N.FLAME_F16):
        assert call(sd=sd, flags=N.FLAME_ONEBIT_BASE) == N.FLAME_ENOTSUP and b"flame_onebit_pack" in err() and b"FLAME_ONEBIT_BASE" in err()


@pytest.mark.parametrize("other", [{"mx": "e4m3"}, {"sparse": 0.01}, {"lowrank": 4}])
def test_encoder_takes_one_downlink(other):
    with pytest.raises(ValueError, match="choose one"):
        egress.MessageEncoder(pin=False, sign=True, **other)
