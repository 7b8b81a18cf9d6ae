"""flame_amd.mx with fmt="e2m1" (the trainer-side MXFP4 format) against tests/mxfp4_ref.py, a numpy
restatement by integer bit manipulation.  CPU only, no native code."""
import collections
import math
import pickle

import cloudpickle
import numpy as np
import pytest
import torch

import mxfp4_ref as R
from flame_amd import mx

F4 = torch.float4_e2m1fn_x2
INF, NAN = float("inf"), float("nan")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_f32(name, got, want):
    """Bitwise, signs of zero included; a NaN equals a NaN."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), name
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), name


def _check(name, x, **kw):
    x = torch.as_tensor(x, dtype=torch.float32) if not isinstance(x, torch.Tensor) else x
    m = mx.quantize({"x": x}, "e2m1", **kw)
    n = x.numel()
    assert isinstance(m, mx.MXWeights) and m.block == 32
    assert m["x"].dtype == F4 and m["x"].shape == (-(-n // 2),)                  # 1-D, packed
    assert m.shapes == {"x": tuple(x.shape)}
    assert m.scales["x"].dtype == torch.uint8 and m.scales["x"].shape == (-(-n // 32),)
    q, s = R.quantize(x.to(torch.float32).numpy())
    got = m["x"].view(torch.uint8).numpy()
    assert np.array_equal(got, q), (name, np.flatnonzero(got != q)[:8])
    assert np.array_equal(m.scales["x"].numpy(), s), name
    if n % 2:
        assert got[-1] >> 4 == 0, name                                            # the pad nibble
    d = mx.dequantize(m)["x"]
    assert d.dtype == torch.float32 and d.shape == x.shape
    _same_f32(name, d.numpy(), R.dequantize(got, s, n))
    return m, d


# ---------------------------------------------------------------------------- the format
def test_codes_and_every_byte_scale_pair():
    assert R.decode_e2m1(np.arange(16)).tolist() == list(mx.E2M1_VALUES)
    assert _bits(R.decode_e2m1(np.arange(16)))[8] == 0x80000000                  # code 8 is -0
    assert mx.FORMATS["e2m1"] == (F4, 2, 6.0)
    # all 256 bytes x 256 scales: 512 elements per scale byte = 16 blocks of one scale
    b = np.tile(np.arange(256, dtype=np.uint8), 256)
    s = np.repeat(np.arange(256, dtype=np.uint8), 16)
    d = mx.dequantize_tensor(torch.from_numpy(b).view(F4), torch.from_numpy(s))
    assert d.shape == (2 * 65536,)
    want = R.dequantize(b, s, 2 * 65536)
    _same_f32("pairs", d.numpy(), want)
    # the products: 16 codes x 256 scales, none rounded
    p = want.reshape(256, 256, 2)[:, :16, 0]                                     # [scale, low nibble = code]
    assert np.isnan(p[255]).all() and np.isfinite(p[:253]).all()
    exact = R.decode_e2m1(np.arange(16)).astype(np.float64)[None, :] * 2.0 ** (np.arange(255, dtype=np.float64)[:, None] - 127)
    fin = np.isfinite(p[:255])
    assert np.array_equal(p[:255][fin].astype(np.float64), exact[fin])
    assert int(np.isinf(p[:255]).sum()) == 12 and int(fin.sum()) == 4068
    sub = fin & (np.abs(p[:255]) < 2.0 ** -126) & (p[:255] != 0)
    assert int(sub.sum()) == 8


# ---------------------------------------------------------------------------- quantize / dequantize
@pytest.mark.parametrize("numel", [1, 2, 31, 32, 33, 63, 70])
def test_random_blocks(numel):
    g = torch.Generator().manual_seed(numel)
    for p in (-40, -13, 0, 5, 30):
        _check(f"{numel}/2^{p}", torch.randn(numel, generator=g) * 2.0 ** p)
    x = torch.randn(70, generator=g) * torch.tensor([2.0 ** -40] * 32 + [1.0] * 32 + [2.0 ** 30] * 6)
    _check("per-block", x)


def test_ties_go_to_the_even_mantissa_bit():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    for k in (-30, 0, 9):
        x = [t * 2.0 ** k for t in ties] + [-t * 2.0 ** k for t in ties] + [4.0 * 2.0 ** k] + [0.0] * 17
        m, d = _check(f"ties/{k}", x)
        assert m.scales["x"].tolist() == [127 + k]
        assert d[:14].tolist() == [w * 2.0 ** k for w in want] + [-w * 2.0 ** k for w in want]
        assert _bits(d.numpy())[7] == 0x80000000                                 # -0.25 * 2^k rounds to -0
    # a hair to either side of a tie
    for t, lo, hi in zip(ties, [0, .5, 1, 1.5, 2, 3, 4], [.5, 1, 1.5, 2, 3, 4, 6]):
        below, above = float(np.nextafter(np.float32(t), np.float32(0))), float(np.nextafter(np.float32(t), np.float32(9)))
        _, d = _check(f"near/{t}", [below, above, -below, -above, 4.0] + [0.0] * 27)
        assert d[:4].tolist() == [lo, hi, -lo, -hi]


def test_saturation_band_and_infinities():
    for k in (-20, -1, 0, 3, 40):
        for frac in (0.01, 0.5, 0.99):
            a = (6.0 + 2.0 * frac) * 2.0 ** k                                    # amax in (6, 8) * 2^e
            m, d = _check(f"sat/{k}/{frac}", [a, -a, a / 3] + [0.0] * 29)
            assert m.scales["x"].tolist() == [127 + k]
            assert d[:2].tolist() == [6.0 * 2.0 ** k, -6.0 * 2.0 ** k]
    m, d = _check("inf", [INF, -INF, 1.0] + [0.0] * 29)
    assert m.scales["x"].tolist() == [125] and d[:3].tolist() == [1.5, -1.5, 0.25 * 4]
    m, d = _check("inf only", [INF, -INF] * 16)
    assert m.scales["x"].tolist() == [127] and d.tolist() == [6.0, -6.0] * 16


def test_a_nan_block_is_scale_byte_255():
    x = torch.arange(96, dtype=torch.float32) - 48
    x[40] = NAN
    m, d = _check("nan", x)
    assert m.scales["x"].tolist()[1] == 255 and 255 not in (m.scales["x"][0], m.scales["x"][2])
    assert torch.isnan(d[32:64]).all() and torch.isfinite(d[:32]).all() and torch.isfinite(d[64:]).all()
    codes = R.unpack(m["x"].view(torch.uint8).numpy(), 96)
    assert codes[40] == 0                                                         # the nibble where x is NaN
    clean = x.clone()
    clean[40] = 0.0
    m2, d2 = _check("clean", clean)
    assert torch.equal(d2[:32], d[:32]) and torch.equal(d2[64:], d[64:])        # the neighbours are untouched
    m, d = _check("all nan", [NAN] * 32)
    assert m.scales["x"].tolist() == [255] and not m["x"].view(torch.uint8).any()
    m, d = _check("nan and inf", [NAN, INF, -INF] + [NAN] * 29)
    assert m.scales["x"].tolist() == [255]


def test_zeros():
    m, d = _check("zeros", [0.0] * 32)
    assert m.scales["x"].tolist() == [127] and not m["x"].view(torch.uint8).any()
    m, d = _check("signed zeros", [0.0, -0.0] * 16)
    assert m.scales["x"].tolist() == [127] and m["x"].view(torch.uint8).tolist() == [0x80] * 16
    assert _bits(d.numpy()).tolist() == [0, 0x80000000] * 16


def test_exponent_clamps():
    for a in (2.0 ** -126, 1.5 * 2.0 ** -126, 2.0 ** -130, 2.0 ** -149, 3 * 2.0 ** -140, 2.0 ** -120 * 1.75):
        m, _ = _check(f"tiny/{a}", [a, -a / 2, a / 4] + [0.0] * 29)
        assert m.scales["x"].tolist() == [max(int(np.floor(np.log2(a))) - 2, -127) + 127]
    assert mx.quantize({"x": torch.tensor([2.0 ** -149])}, "e2m1").scales["x"].tolist() == [0]
    big = float(np.finfo(np.float32).max)
    for a in (big, 2.0 ** 127, 1.25 * 2.0 ** 126, 2.0 ** 120):
        m, d = _check(f"huge/{a}", [a, -a, a / 2, 1.0] + [0.0] * 28)
        assert m.scales["x"].tolist() == [int(np.floor(np.log2(a))) - 2 + 127]
        assert torch.isfinite(d).all()
    assert mx.quantize({"x": torch.tensor([big])}, "e2m1").scales["x"].tolist() == [252]      # the top: 2^125


def test_odd_numel_partial_block_and_2d():
    g = torch.Generator().manual_seed(2)
    for shape in [(1,), (3,), (33,), (65,), (3, 37), (5, 1, 7), (2, 48)]:
        m, d = _check(f"shape/{shape}", torch.randn(*shape, generator=g) * 5)
        n = math.prod(shape)
        assert m["x"].numel() == (n + 1) // 2 and m.scales["x"].numel() == (n + 31) // 32


def test_idempotent():
    g = torch.Generator().manual_seed(11)
    w = {"a": torch.randn(70, generator=g), "b": torch.randn(4, 33, generator=g) * 1e-5,
         "c": torch.tensor([0.0, -0.0, 6.0, 7.9, 2.0 ** -149, 1e38, INF] + [1.0] * 26),
         "n": torch.tensor([NAN, 3.0] + [1.0] * 62)}
    m = mx.quantize(w, "e2m1")
    deq = mx.dequantize(m)
    again = mx.quantize(deq, "e2m1")
    for k in w:
        assert again.shapes[k] == m.shapes[k] == tuple(w[k].shape)
        _same_f32(k, mx.dequantize(again)[k].numpy(), deq[k].numpy())             # the value, NaN blocks included
        assert torch.equal(again.scales[k], m.scales[k]), k
        if k != "n":                                                              # (a NaN block's nibbles become 0)
            assert torch.equal(again[k].view(torch.uint8), m[k].view(torch.uint8)), k


def test_error_bound():
    """With X = 2^e the block's scale (e unclamped): the grid's widest gap is 2 (4 to 6), so inside
    [-6, 6] X the nearest point is at most 1 X away; amax < 8 X, so the clamp at 6 X costs less than 2 X."""
    g = torch.Generator().manual_seed(7)
    for p in (0, -14, -100, 83):
        x = torch.randn(4096, generator=g) * 2.0 ** p * torch.exp(torch.randn(4096, generator=g) * 3)
        m = mx.quantize({"x": x}, "e2m1")
        s = m.scales["x"].numpy()
        assert s.min() > 0 and s.max() < 253                                      # no clamp in this sweep
        d = mx.dequantize(m)["x"].double()
        X = torch.from_numpy(R.decode_e8m0(s).astype(np.float64)).repeat_interleave(32)
        err = (d - x.double()).abs()
        assert bool((err < 2 * X).all()), p
        inside = x.double().abs() <= 6 * X
        assert bool((err[inside] <= X[inside]).all()) and bool(inside.any()) and bool((~inside).any()), p


def test_input_dtypes_and_passthrough():
    g = torch.Generator().manual_seed(3)
    w = collections.OrderedDict([("w", torch.randn(3, 41, generator=g)), ("h", torch.randn(65, generator=g).to(torch.bfloat16)),
                                 ("f", torch.randn(33, generator=g).to(torch.float16)), ("small", torch.randn(5, generator=g)),
                                 ("nbt", torch.tensor(7)), ("mask", torch.tensor([True, False])),
                                 ("d", torch.randn(64, generator=g, dtype=torch.float64)),
                                 ("u8", torch.arange(40, dtype=torch.uint8))])
    m = mx.quantize(w, "e2m1", min_numel=6)
    assert list(m.keys()) == list(w.keys())
    assert sorted(m.scales) == sorted(m.shapes) == ["f", "h", "w"]
    for k in ("small", "nbt", "mask", "d", "u8"):
        assert m[k] is w[k]
    for k in ("w", "h", "f"):       # computed in fp32: the same bytes as the fp32 copy's
        q, s = R.quantize(w[k].to(torch.float32).numpy())
        assert np.array_equal(m[k].view(torch.uint8).numpy(), q) and np.array_equal(m.scales[k].numpy(), s)
        assert m.shapes[k] == tuple(w[k].shape) and m[k].dim() == 1
    d = mx.dequantize(m)
    assert d["nbt"] is w["nbt"] and d["w"].dtype == d["h"].dtype == torch.float32 and d["w"].shape == (3, 41)
    assert list(mx.quantize(w, "e2m1", min_numel=10 ** 6).scales) == []
    assert mx.quantize(w, "e4m3").shapes == {}                                    # float8 keys keep their own shape
    with pytest.raises(ValueError, match="fmt"):
        mx.quantize(w, "e3m0")


def _intact(a, b):
    assert type(b) is mx.MXWeights and list(a.keys()) == list(b.keys()) and sorted(a.scales) == sorted(b.scales)
    assert a.shapes == b.shapes
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
        raw = torch.uint8 if k in a.scales else a[k].dtype
        assert torch.equal(a[k].view(raw), b[k].view(raw)), k
    for k in a.scales:
        assert b.scales[k].dtype == torch.uint8 and torch.equal(a.scales[k], b.scales[k])


def test_pickle_round_trips():
    g = torch.Generator().manual_seed(5)
    m = mx.quantize(collections.OrderedDict([("w", torch.randn(3, 41, generator=g)), ("nbt", torch.tensor(9)),
                                             ("v", torch.randn(33, generator=g))]), "e2m1")
    assert m.shapes == {"w": (3, 41), "v": (33,)}
    _intact(m, pickle.loads(pickle.dumps(m)))
    _intact(m, cloudpickle.loads(cloudpickle.dumps(m)))
    _intact(m, m.to("cpu"))
    fn, args = m.__reduce__()
    assert fn is mx.MXWeights and len(args) == 4 and args[1] is m.scales and args[2] == {"w": "e2m1", "v": "e2m1"}
    assert args[3] == m.shapes and args[0]["w"].dtype == torch.uint8


class _ParentLayout:
    """Pickles as an MXWeights did before ``shapes``: three constructor arguments."""

    def __init__(self, m):
        self.m = m

    def __reduce__(self):
        fn, args = self.m.__reduce__()
        return fn, args[:3]


def test_a_three_argument_pickle_still_loads():
    g = torch.Generator().manual_seed(6)
    m = mx.quantize(collections.OrderedDict([("w", torch.randn(3, 40, generator=g)), ("nbt", torch.tensor(9))]), "e5m2")
    back = pickle.loads(pickle.dumps(_ParentLayout(m)))
    _intact(m, back)
    assert back.shapes == {} and back["w"].dtype == torch.float8_e5m2 and back["w"].shape == (3, 40)
