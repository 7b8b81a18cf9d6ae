"""MXFP8 and MXFP4 updates: the trainer-side formats of the 8-bit and 4-bit uplinks (torch only, no
native code).

An MX update (OCP Microscaling v1.0, "MXFP8") holds a quantised float key as one OCP ``e4m3fn`` or
``e5m2`` byte per element plus one E8M0 power-of-two scale byte per block of 32 flat C-order elements:
1 + 1/32 bytes per parameter, x0.258 of fp32 and x0.516 of bf16.  The block scale is what makes fp8
usable for model deltas (a raw e4m3 cast has nothing below 2^-9).

An MXFP4 update (``fmt="e2m1"``) holds one 4-bit OCP ``e2m1`` code per element instead (0, 0.5, 1,
1.5, 2, 3, 4, 6 and their negatives; no inf, no NaN), two per byte -- flat element ``2i`` the low nibble
of byte ``i``, ``2i + 1`` the high one, ``torch.float4_e2m1fn_x2``'s order -- under the same scale
bytes: 1/2 + 1/32 bytes per parameter, x0.133 of fp32 and x0.515 of MXFP8.  A quantised e2m1 key is a
1-D tensor of ``ceil(numel / 2)`` bytes (an odd ``numel``'s last high nibble is a zero pad); its
logical shape lives in ``MXWeights.shapes``.  e2m1 has no NaN, so a block that holds one gets scale
byte 255 and dequantises to NaN as a whole.

    from flame_amd import mx
    weights = mx.quantize(delta)            # trainer: an MXWeights, sent as the update
    fp32 = mx.dequantize(weights)           # the update's value, by definition

``dequantize`` is the contract: an element's value is ``f32(q) * f32(scale of its block)``, one
fp32 multiply.  The aggregator's kernels (``flame_agg_reduce_mx``, ``flame_agg_reduce_mxfp4``) sum exactly these values, so a
round over MX updates equals the same round over their dequantised fp32 copies bit for bit.
"""
from __future__ import annotations

import collections
import math

import torch

BLOCK = 32
# name -> (element dtype, emax: exponent of the largest power of two, largest finite value)
FORMATS = {"e4m3": (torch.float8_e4m3fn, 8, 448.0), "e5m2": (torch.float8_e5m2, 15, 57344.0),
           "e2m1": (torch.float4_e2m1fn_x2, 2, 6.0)}
PACKED = torch.float4_e2m1fn_x2         # the one element dtype that holds two elements per byte
# the value of an e2m1 code: sign, two exponent bits, one mantissa bit
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)
ELEMENT_DTYPES = tuple(f[0] for f in FORMATS.values())
QUANTIZED_FROM = (torch.float32, torch.bfloat16, torch.float16)


def n_blocks(numel: int) -> int:
    return -(-numel // BLOCK)


class MXWeights(dict):
    """One trainer's update.  A quantised key holds a float8 tensor of the key's own shape, or a 1-D
    ``float4_e2m1fn_x2`` tensor of ``ceil(numel / 2)`` bytes; every other key the plain tensor it
    always held.  ``scales``: ``{key: uint8 [ceil(numel / 32)]}``, the E8M0 bytes; block ``b`` covers
    flat elements ``[32b, 32b + 32)``, the last block may be partial.  ``shapes``: ``{key: logical
    shape}`` of the e2m1 keys alone (a float8 key keeps its own shape)."""

    block = BLOCK

    def __init__(self, weights=(), scales=None, formats=None, shapes=None):
        super().__init__(weights)
        self.scales = dict(scales) if scales is not None else {}
        self.shapes = {k: tuple(v) for k, v in shapes.items()} if shapes is not None else {}
        for k, fmt in (formats or {}).items():      # unpickling: the element bytes travelled as uint8
            self[k] = self[k].view(FORMATS[fmt][0])

    def __reduce__(self):
        # torch's plain-pickle path does not take float8 / float4 tensors back (its legacy loader asks the
        # untyped storage for a dtype), so the element bytes travel as uint8 views and ``formats``
        # names each key's element format; the scales are uint8 already
        names = {dt: fmt for fmt, (dt, _, _) in FORMATS.items()}
        formats = {k: names[v.dtype] for k, v in self.items() if isinstance(v, torch.Tensor) and v.dtype in names}
        return (MXWeights, ({k: v.view(torch.uint8) if k in formats else v for k, v in self.items()},
                            self.scales, formats, self.shapes))

    def _map(self, f):
        # (a packed key moves as its bytes: torch implements few operations on the float4 shell dtype)
        g = lambda v: f(v.view(torch.uint8)).view(PACKED) if v.dtype == PACKED else f(v)     # noqa: E731
        return MXWeights(((k, g(v) if isinstance(v, torch.Tensor) else v) for k, v in self.items()),
                         {k: f(s) for k, s in self.scales.items()}, shapes=self.shapes)

    def to(self, device, non_blocking: bool = False):
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def pin_memory(self):
        return self._map(lambda t: t.pin_memory())


def _blocks(x: torch.Tensor):
    """``x`` as fp32 blocks [ceil(numel / 32), 32], zero-padded."""
    flat = x.detach().reshape(-1).to(torch.float32)
    nb = n_blocks(flat.numel())
    if nb * BLOCK != flat.numel():
        flat = torch.cat([flat, flat.new_zeros(nb * BLOCK - flat.numel())])
    return flat.view(nb, BLOCK)


def _quantize_e2m1(x: torch.Tensor):
    """(1-D float4_e2m1fn_x2 [ceil(numel / 2)], uint8 scales) of ``x``, by the rule of DESIGN.md §2."""
    _, emax, fmax = FORMATS["e2m1"]
    n = x.numel()
    blk = _blocks(x)
    mag = blk.abs()
    amax = torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag)).amax(dim=1)     # the largest finite |x|
    _, ex = torch.frexp(amax)
    e = (ex.to(torch.int32) - 1 - emax).clamp(-127, 127)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    a = torch.ldexp(blk, -e.unsqueeze(1)).abs().clamp(max=fmax)     # saturating: +-inf and (6, 8) * 2^e become 6
    # round to nearest, ties to the even mantissa bit: the comparisons at the seven midpoints (a NaN is code 0)
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    nan = torch.isnan(blk)
    code = code + (torch.signbit(blk) & ~nan).to(torch.uint8) * 8   # the sign is kept, -0 included
    # e2m1 has no NaN: the block's scale byte says it, for every element of the block
    sb = torch.where(nan.any(dim=1), torch.full_like(e, 255), e + 127).to(torch.uint8)
    code = code.view(-1)[:n]
    if n % 2:
        code = torch.cat([code, code.new_zeros(1)])                 # the pad nibble
    packed = code[0::2] | (code[1::2] << 4)
    return packed.contiguous().view(PACKED), sb


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
    ("e4m3", "e5m2" or "e2m1").  fp32 / bf16 / f16 keys of at least ``min_numel`` elements are quantised
    (computed in fp32); every other key passes through unchanged.  Runs where the tensors live."""
    if fmt not in FORMATS:
        raise ValueError(f"flame_amd.mx.quantize: fmt {fmt!r} is not one of {sorted(FORMATS)}")
    out, scales, shapes = collections.OrderedDict(), {}, {}
    for k, v in weights.items():
        if isinstance(v, torch.Tensor) and v.dtype in QUANTIZED_FROM and v.numel() >= max(min_numel, 1):
            if fmt == "e2m1":
                out[k], scales[k] = _quantize_e2m1(v)
                shapes[k] = tuple(v.shape)
            else:
                out[k], scales[k] = _quantize_tensor(v, fmt)
        else:
            out[k] = v
    return MXWeights(out, scales, shapes=shapes)


def dequantize_tensor(q: torch.Tensor, s: torch.Tensor, shape=None) -> torch.Tensor:
    """The value of one quantised key: ``f32(q) * f32(scale of the element's block)``.  ``shape``: the
    logical shape of a packed e2m1 key (default: every nibble, 1-D)."""
    if q.dtype == PACKED:
        b = q.reshape(-1).view(torch.uint8)
        n = 2 * b.numel() if shape is None else math.prod(shape)
        code = torch.stack([b & 15, b >> 4], dim=1).reshape(-1)[:n]
        x = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=q.device)[code.long()]
        sf = s.view(torch.float8_e8m0fnu).to(torch.float32).repeat_interleave(BLOCK)[:n]
        return (x * sf).reshape((n,) if shape is None else tuple(shape))
    sf = s.view(torch.float8_e8m0fnu).to(torch.float32).repeat_interleave(BLOCK)[:q.numel()]
    return (q.reshape(-1).to(torch.float32) * sf).reshape(q.shape)


def dequantize(mx: MXWeights) -> dict:
    """``{key: fp32 tensor}`` for the quantised keys of ``mx``, every other key as it is.  THE
    definition of an MX update's value: one fp32 multiply per element."""
    out = collections.OrderedDict()
    for k, v in mx.items():
        out[k] = dequantize_tensor(v, mx.scales[k], mx.shapes.get(k)) if k in mx.scales else v
    return out
