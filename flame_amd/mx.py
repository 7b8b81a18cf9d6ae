"""MXFP8 updates: the trainer-side format of the 8-bit uplink (torch only, no native code).

An MX update (OCP Microscaling v1.0, "MXFP8") holds a quantised float key as one OCP ``e4m3fn`` or
``e5m2`` byte per element plus one E8M0 power-of-two scale byte per block of 32 flat C-order elements:
1 + 1/32 bytes per parameter, x0.258 of fp32 and x0.516 of bf16.  The block scale is what makes fp8
usable for model deltas (a raw e4m3 cast has nothing below 2^-9).

    from flame_amd import mx
    weights = mx.quantize(delta)            # trainer: an MXWeights, sent as the update
    fp32 = mx.dequantize(weights)           # the update's value, by definition

``dequantize`` is the contract: an element's value is ``f32(q) * f32(scale of its block)``, one
fp32 multiply.  The aggregator's kernel (``flame_agg_reduce_mx``) sums exactly these values, so a
round over MX updates equals the same round over their dequantised fp32 copies bit for bit.
"""
from __future__ import annotations

import collections

import torch

BLOCK = 32
# name -> (element dtype, emax: exponent of the largest power of two, largest finite value)
FORMATS = {"e4m3": (torch.float8_e4m3fn, 8, 448.0), "e5m2": (torch.float8_e5m2, 15, 57344.0)}
ELEMENT_DTYPES = tuple(f[0] for f in FORMATS.values())
QUANTIZED_FROM = (torch.float32, torch.bfloat16, torch.float16)


def n_blocks(numel: int) -> int:
    return -(-numel // BLOCK)


class MXWeights(dict):
    """One trainer's update.  A quantised key holds a float8 tensor of the key's own shape, every
    other key the plain tensor it always held.  ``scales``: ``{key: uint8 [ceil(numel / 32)]}``, the
    E8M0 bytes; block ``b`` covers flat elements ``[32b, 32b + 32)``, the last block may be partial."""

    block = BLOCK

    def __init__(self, weights=(), scales=None, formats=None):
        super().__init__(weights)
        self.scales = dict(scales) if scales is not None else {}
        for k, fmt in (formats or {}).items():      # unpickling: the element bytes travelled as uint8
            self[k] = self[k].view(FORMATS[fmt][0])

    def __reduce__(self):
        # torch's plain-pickle path does not take float8 tensors back (its legacy loader asks the
        # untyped storage for a dtype), so the element bytes travel as uint8 views and ``formats``
        # names each key's element format; the scales are uint8 already
        names = {dt: fmt for fmt, (dt, _, _) in FORMATS.items()}
        formats = {k: names[v.dtype] for k, v in self.items() if isinstance(v, torch.Tensor) and v.dtype in names}
        return (MXWeights, ({k: v.view(torch.uint8) if k in formats else v for k, v in self.items()},
                            self.scales, formats))

    def _map(self, f):
        return MXWeights(((k, f(v) if isinstance(v, torch.Tensor) else v) for k, v in self.items()),
                         {k: f(s) for k, s in self.scales.items()})

    def to(self, device, non_blocking: bool = False):
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def pin_memory(self):
        return self._map(lambda t: t.pin_memory())


def _quantize_tensor(x: torch.Tensor, fmt: str):
    dt, emax, fmax = FORMATS[fmt]
    flat = x.detach().reshape(-1).to(torch.float32)
    n = flat.numel()
    nb = n_blocks(n)
    if nb * BLOCK != n:
        flat = torch.cat([flat, flat.new_zeros(nb * BLOCK - n)])
    blk = flat.view(nb, BLOCK)
    mag = blk.abs()
    amax = torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag)).amax(dim=1)     # the largest finite |x|
    _, ex = torch.frexp(amax)                           # amax = m * 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = (ex.to(torch.int32) - 1 - emax).clamp(-127, 127)
    e = torch.where(amax > 0, e, torch.zeros_like(e))   # an all-zero block, or one without a finite element: 2^0
    q = torch.ldexp(blk, -e.unsqueeze(1))               # a power of two: exact
    q = q.clamp(-fmax, fmax)                            # saturating, as the OCP conversion is; a NaN stays a NaN
    q = q.to(dt).view(-1)[:n].reshape(x.shape)          # round to nearest even
    return q, (e + 127).to(torch.uint8)


def quantize(weights, fmt: str = "e4m3", min_numel: int = 0) -> MXWeights:
    """``weights`` (a state_dict-style mapping) as an :class:`MXWeights` in element format ``fmt``
    ("e4m3" or "e5m2").  fp32 / bf16 / f16 keys of at least ``min_numel`` elements are quantised
    (computed in fp32); every other key passes through unchanged.  Runs where the tensors live."""
    if fmt not in FORMATS:
        raise ValueError(f"flame_amd.mx.quantize: fmt {fmt!r} is not one of {sorted(FORMATS)}")
    out, scales = collections.OrderedDict(), {}
    for k, v in weights.items():
        if isinstance(v, torch.Tensor) and v.dtype in QUANTIZED_FROM and v.numel() >= max(min_numel, 1):
            out[k], scales[k] = _quantize_tensor(v, fmt)
        else:
            out[k] = v
    return MXWeights(out, scales)


def dequantize_tensor(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The value of one quantised key: ``f32(q) * f32(scale of the element's block)``."""
    sf = s.view(torch.float8_e8m0fnu).to(torch.float32).repeat_interleave(BLOCK)[:q.numel()]
    return (q.reshape(-1).to(torch.float32) * sf).reshape(q.shape)


def dequantize(mx: MXWeights) -> dict:
    """``{key: fp32 tensor}`` for the quantised keys of ``mx``, every other key as it is.  THE
    definition of an MX update's value: one fp32 multiply per element."""
    out = collections.OrderedDict()
    for k, v in mx.items():
        out[k] = dequantize_tensor(v, mx.scales[k]) if k in mx.scales else v
    return out
