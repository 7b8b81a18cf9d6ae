"""flame_amd.mx (the trainer-side MXFP8 format) against tests/mx_ref.py, a numpy restatement by integer
bit manipulation that uses none of torch's float8 casts.  CPU only, no native code."""
import collections
import pickle

import cloudpickle
import numpy as np
import pytest
import torch

import mx_ref as R
from flame_amd import mx

FMTS = ["e4m3", "e5m2"]
DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
TOP = {"e4m3": 448.0, "e5m2": 57344.0}
SUB_STEP = {"e4m3": 2.0 ** -10, "e5m2": 2.0 ** -17}     # half the subnormal step of an element, in units of the scale


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_f32(name, got, want):
    """Bitwise, signs of zero included; a NaN equals a NaN."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), name
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), name


def _same_bytes(name, got, want, fmt):
    """Element bytes equal; where the reference holds a NaN any NaN byte of the format will do."""
    got, want = np.asarray(got, np.uint8).reshape(-1), np.asarray(want, np.uint8).reshape(-1)
    nan = np.isnan(R.decode(want, fmt))
    assert np.array_equal(np.isnan(R.decode(got, fmt)), nan), name
    assert np.array_equal(got[~nan], want[~nan]), (name, np.flatnonzero(got != want)[:8])


def _check(name, x, fmt):
    x = torch.as_tensor(x, dtype=torch.float32)
    m = mx.quantize({"x": x}, fmt)
    assert isinstance(m, mx.MXWeights) and m.block == 32
    assert m["x"].dtype == DT[fmt] and m["x"].shape == x.shape
    assert m.scales["x"].dtype == torch.uint8 and m.scales["x"].shape == (-(-x.numel() // 32),)
    q, s = R.quantize(x.numpy(), fmt)
    _same_bytes(name, m["x"].view(torch.uint8).numpy(), q, fmt)
    assert np.array_equal(m.scales["x"].numpy(), s), name
    assert 255 not in s
    d = mx.dequantize(m)["x"]
    assert d.dtype == torch.float32 and d.shape == x.shape
    _same_f32(name, d.numpy(), R.dequantize(m["x"].view(torch.uint8).numpy(), s, fmt))
    return m, d


# ---------------------------------------------------------------------------- the three byte formats
def test_every_byte_decodes_as_torch_does():
    b = np.arange(256, dtype=np.uint8)
    for fmt in FMTS:
        _same_f32(fmt, torch.from_numpy(b.copy()).view(DT[fmt]).to(torch.float32).numpy(), R.decode(b, fmt))
    _same_f32("e8m0", torch.from_numpy(b.copy()).view(torch.float8_e8m0fnu).to(torch.float32).numpy(), R.decode_e8m0(b))
    assert _bits(R.decode_e8m0(b))[0] == 0x00400000 and np.isnan(R.decode_e8m0(b)[255])


# ---------------------------------------------------------------------------- quantize / dequantize
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("numel", [1, 31, 32, 33, 70])
def test_random_blocks(fmt, numel):
    g = torch.Generator().manual_seed(numel)
    for scale in (1.0, 1e-3, 37.0, 1e-20, 1e20):
        _check(f"{fmt}/{numel}/{scale}", torch.randn(numel, generator=g) * scale, fmt)
    # every block at another magnitude
    x = torch.randn(70, generator=g) * torch.tensor([1e-6] * 32 + [1.0] * 32 + [1e6] * 6)
    _check(f"{fmt}/per-block", x, fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_special_values(fmt):
    inf, nan = float("inf"), float("nan")
    sub = float(np.float32(2.0 ** -149))
    blocks = {
        "zeros": [0.0] * 32,
        "signed zeros": [0.0, -0.0] * 16,
        "nans": [nan] * 32,
        "infs": [inf, -inf] * 16,
        "subnormals": [sub, -sub, sub * 5, 2.0 ** -127, -(2.0 ** -130)] + [0.0] * 27,
        "mixed": [0.0, -0.0, sub, inf, -inf, nan, 1.5, -3.25, 1e-3] + [0.125] * 23,
        "nan and inf only": [nan, inf, -inf, nan] + [nan] * 28,
    }
    for name, vals in blocks.items():
        m, d = _check(f"{fmt}/{name}", vals, fmt)
        x = torch.tensor(vals)
        fin = torch.isfinite(x)
        assert torch.isnan(d[torch.isnan(x)]).all()                                   # a NaN stays a NaN
        assert torch.isfinite(d[~torch.isnan(x)]).all()                               # +-inf saturates
        if not fin.any() or x[fin].abs().max() == 0:
            assert m.scales["x"].tolist() == [127], name
    m, d = _check(f"{fmt}/inf", [inf, -inf, 1.0] + [0.0] * 29, fmt)
    s = float(R.decode_e8m0(m.scales["x"].numpy())[0])
    assert d[:2].tolist() == [TOP[fmt] * s, -TOP[fmt] * s]


@pytest.mark.parametrize("fmt", FMTS)
def test_saturation_band(fmt):
    """amax in (top, 2^(emax + 1)) * 2^k: beyond the largest finite element after scaling, so the clamp
    saturates it (torch's own e4m3 cast would give NaN from 480 on)."""
    lo, hi = TOP[fmt], 2.0 * 2.0 ** R.FMT[fmt][3]
    for k in (-20, -1, 0, 3, 40):
        for frac in (0.01, 0.5, 0.99):
            a = (lo + (hi - lo) * frac) * 2.0 ** k
            m, d = _check(f"{fmt}/sat/{k}/{frac}", [a, -a, a / 3] + [0.0] * 29, fmt)
            assert m.scales["x"].tolist() == [127 + k]
            assert d[:2].tolist() == [lo * 2.0 ** k, -lo * 2.0 ** k]


@pytest.mark.parametrize("fmt", FMTS)
def test_exponent_clamps(fmt):
    emax = R.FMT[fmt][3]
    for a in (2.0 ** -126, 1.5 * 2.0 ** -126, 2.0 ** -130, 2.0 ** -149, 3 * 2.0 ** -140, 2.0 ** -120 * 1.75):
        m, _ = _check(f"{fmt}/tiny/{a}", [a, -a / 2, a / 4] + [0.0] * 29, fmt)
        assert m.scales["x"].tolist() == [max(int(np.floor(np.log2(a))) - emax, -127) + 127]
    assert mx.quantize({"x": torch.tensor([2.0 ** -149])}, fmt).scales["x"].tolist() == [0]
    big = float(np.finfo(np.float32).max)
    for a in (big, 2.0 ** 127, 1.25 * 2.0 ** 126, 2.0 ** 120):
        m, _ = _check(f"{fmt}/huge/{a}", [a, -a, a / 2, 1.0] + [0.0] * 28, fmt)
        assert m.scales["x"].tolist() == [int(np.floor(np.log2(a))) - emax + 127]


@pytest.mark.parametrize("fmt", FMTS)
def test_error_bound(fmt):
    """|d - x| <= |x| / 8 + X * 2^-10 (e4m3) / X * 2^-17 (e5m2), X the block's scale: 3 / 2 mantissa bits
    give a relative half-ulp of 2^-4 / 2^-3, the subnormal step an absolute one, and the clamp at most
    1/8 of the value (448 against < 512, 57344 against < 65536)."""
    g = torch.Generator().manual_seed(7)
    for scale in (1.0, 1e-4, 1e-30, 1e25):
        x = torch.randn(4096, generator=g) * scale * torch.exp(torch.randn(4096, generator=g) * 3)
        m = mx.quantize({"x": x}, fmt)
        d = mx.dequantize(m)["x"].double()
        X = torch.from_numpy(R.decode_e8m0(m.scales["x"].numpy()).astype(np.float64)).repeat_interleave(32)
        bound = x.double().abs() / 8 + X * SUB_STEP[fmt]
        assert bool(((d - x.double()).abs() <= bound).all()), (fmt, scale)


@pytest.mark.parametrize("fmt", FMTS)
def test_requantize_is_identity(fmt):
    g = torch.Generator().manual_seed(11)
    w = {"a": torch.randn(70, generator=g), "b": torch.randn(4, 33, generator=g) * 1e-5,
         "c": torch.tensor([0.0, -0.0, 448.0, 57344.0, 2.0 ** -149, 1e38] + [1.0] * 30)}
    m = mx.quantize(w, fmt)
    again = mx.quantize(mx.dequantize(m), fmt)
    for k in w:
        assert torch.equal(again[k].view(torch.uint8), m[k].view(torch.uint8)), k
        assert torch.equal(again.scales[k], m.scales[k]), k


def test_input_dtypes_and_passthrough():
    g = torch.Generator().manual_seed(3)
    w = collections.OrderedDict([("w", torch.randn(3, 40, generator=g)), ("h", torch.randn(65, generator=g).to(torch.bfloat16)),
                                 ("f", torch.randn(33, generator=g).to(torch.float16)), ("small", torch.randn(5, generator=g)),
                                 ("nbt", torch.tensor(7)), ("mask", torch.tensor([True, False])),
                                 ("d", torch.randn(64, generator=g, dtype=torch.float64))])
    m = mx.quantize(w, "e5m2", min_numel=6)
    assert list(m.keys()) == list(w.keys())
    assert sorted(m.scales) == ["f", "h", "w"]
    for k in ("small", "nbt", "mask", "d"):
        assert m[k] is w[k]
    for k in ("w", "h", "f"):       # computed in fp32: the same bytes as the fp32 copy's
        q, s = R.quantize(w[k].to(torch.float32).numpy(), "e5m2")
        _same_bytes(k, m[k].view(torch.uint8).numpy(), q, "e5m2")
        assert np.array_equal(m.scales[k].numpy(), s) and m[k].shape == w[k].shape
    d = mx.dequantize(m)
    assert d["nbt"] is w["nbt"] and d["w"].dtype == d["h"].dtype == torch.float32
    assert list(mx.quantize(w, min_numel=10 ** 6).scales) == []
    with pytest.raises(ValueError, match="fmt"):
        mx.quantize(w, "e3m4")


def _intact(a, b):
    assert type(b) is mx.MXWeights and list(a.keys()) == list(b.keys()) and sorted(a.scales) == sorted(b.scales)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
        raw = torch.uint8 if k in a.scales else a[k].dtype
        assert torch.equal(a[k].view(raw), b[k].view(raw)), k
    for k in a.scales:
        assert b.scales[k].dtype == torch.uint8 and torch.equal(a.scales[k], b.scales[k])


@pytest.mark.parametrize("fmt", FMTS)
def test_pickle_round_trips(fmt):
    g = torch.Generator().manual_seed(5)
    m = mx.quantize(collections.OrderedDict([("w", torch.randn(3, 40, generator=g)), ("nbt", torch.tensor(9)),
                                             ("v", torch.randn(33, generator=g))]), fmt)
    _intact(m, pickle.loads(pickle.dumps(m)))
    _intact(m, cloudpickle.loads(cloudpickle.dumps(m)))
    _intact(m, m.to("cpu"))
    fn, args = m.__reduce__()
    assert fn is mx.MXWeights and isinstance(args[0], dict) and args[1] is m.scales
