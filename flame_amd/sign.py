"""Scaled-sign updates: the trainer-side format of the 1-bit uplink (torch only, no native code).

A sign update holds a compressed float key as one bit per element and one fp32 scale per block of
``BLOCK = 256`` elements: the update of signSGD with majority vote (Bernstein et al., ICML 2018), of
EF-signSGD (Karimireddy et al., ICML 2019) and of 1-bit Adam.  That is 0.14 bytes per parameter, against 4
for fp32 and 0.53 for MXFP4.  Sign compression is biased, so a trainer keeps what it did not send:

    from flame_amd import sign
    ef = sign.ErrorFeedback()
    sent = ef.compress(delta)                   # trainer: a SignWeights of delta + residual, sent as the update
    dense = sign.dequantize(sent)               # the update's value: +scale or -scale per element

The contract ("the sign contract"): the aggregate is bit for bit the fp32 round over
``dequantize(update)`` -- per element and in cache order ``acc = f32(acc + f32((+-s) * rate_i))``, no FMA,
denormals kept.  The aggregator's kernel is ``flame_agg_reduce_sign``.

The other direction ("the sign packer"): ``engine.sign_compress`` is ``compress(fold=True)`` on the
device (kernel ``flame_onebit_pack``), ``egress.MessageEncoder(sign=True)`` sends the signs of the model's change
since the last message, and :func:`apply_` is the trainer's side of it.
"""
from __future__ import annotations

import collections
import math

import torch

COMPRESSED_FROM = (torch.float32, torch.bfloat16, torch.float16)
BLOCK = 256         # elements per fp32 scale
WORD = 64           # a key's bits are whole 64-bit words


class SignWeights(dict):
    """One trainer's update.  A compressed key holds its bits, a 1-D uint8 tensor of ``8 * ceil(numel / 64)``
    bytes: element ``e`` is bit ``e % 8`` of byte ``e // 8`` (little-endian: bit ``e % 64`` of 64-bit word
    ``e // 64``), 1 = negative, the pad bits of the last word 0.  Every other key holds the plain tensor it
    always held.  ``scales``: ``{key: fp32 [ceil(numel / 256)]}``, one magnitude per block.  ``shapes``:
    ``{key: logical shape}``."""

    def __init__(self, weights=(), scales=None, shapes=None):
        super().__init__(weights)
        self.scales = dict(scales) if scales is not None else {}
        self.shapes = {k: tuple(v) for k, v in shapes.items()} if shapes is not None else {}

    def __reduce__(self):
        return (SignWeights, (dict(self), self.scales, self.shapes))

    def _map(self, f):
        return SignWeights(((k, f(v) if isinstance(v, torch.Tensor) else v) for k, v in self.items()),
                           {k: f(s) for k, s in self.scales.items()}, self.shapes)

    def to(self, device, non_blocking: bool = False):
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def pin_memory(self):
        return self._map(lambda t: t.pin_memory())


def _pad(flat: torch.Tensor, to: int) -> torch.Tensor:
    n = -(-flat.numel() // to) * to
    return flat if n == flat.numel() else torch.cat([flat, flat.new_zeros(n - flat.numel())])


def fold_scales(x: torch.Tensor) -> torch.Tensor:
    """The block scales of ``x`` in the fold order ("the sign packer"): the block's 256
    magnitudes, the last block zero-padded, halved by ``a = a[:h] + a[h:]`` for ``h = 128, 64, ..., 1`` (each
    one fp32 add), then divided by the block's true length as an fp32.  This is what the device-side packer
    (``flame_onebit_pack``) gives bit for bit.  These statements are the definition."""
    flat = x.detach().reshape(-1)
    n = flat.numel()
    nb = -(-n // BLOCK)
    a = _pad(flat.float().abs(), BLOCK).view(nb, BLOCK)
    while a.shape[1] > 1:
        h = a.shape[1] // 2
        a = a[:, :h] + a[:, h:]
    lengths = torch.full((nb,), float(BLOCK), dtype=torch.float32, device=flat.device)
    lengths[-1] = float(n - (nb - 1) * BLOCK)
    return a.view(nb) / lengths


def compress_tensor(x: torch.Tensor, fold: bool = False):
    """``(bits, scales)`` of one tensor.  Bit ``e`` is ``torch.signbit(x)[e]`` (``-0.0`` gives 1, pad bits 0).
    ``scales[b]`` is the block's mean magnitude: ``x.float().abs()`` summed over the block's elements
    (``torch.sum`` over the zero-padded ``[blocks, 256]`` view, fp32) divided by the block's true length as
    an fp32 tensor.  These statements are the definition.  With ``fold`` the sum is taken in the stated
    order of :func:`fold_scales` instead, which agrees with ``torch.sum`` to fp32 roundoff."""
    flat = x.detach().reshape(-1)
    n = flat.numel()
    neg = _pad(torch.signbit(flat), WORD).view(-1, 8).to(torch.int32)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=flat.device)
    bits = (neg * weights).sum(1).to(torch.uint8)
    if fold:
        return bits, fold_scales(flat)
    nb = -(-n // BLOCK)
    lengths = torch.full((nb,), float(BLOCK), dtype=torch.float32, device=flat.device)
    lengths[-1] = float(n - (nb - 1) * BLOCK)
    scales = _pad(flat.float().abs(), BLOCK).view(nb, BLOCK).sum(1) / lengths
    return bits, scales


def compress(weights, min_numel: int = 0, fold: bool = False) -> SignWeights:
    """``weights`` (a state_dict-style mapping) as a :class:`SignWeights`: fp32 / bf16 / f16 keys of at least
    ``min_numel`` elements (and at least one) are compressed by :func:`compress_tensor`; every other key --
    int, bool, smaller -- passes through unchanged.  Runs where the tensors live.  ``fold``: the scales in
    :func:`fold_scales`' order, as ``engine.sign_compress`` gives them."""
    out, scales, shapes = collections.OrderedDict(), {}, {}
    for k, v in weights.items():
        if isinstance(v, torch.Tensor) and v.dtype in COMPRESSED_FROM and v.numel() >= max(min_numel, 1):
            out[k], scales[k] = compress_tensor(v, fold)
            shapes[k] = tuple(v.shape)
        else:
            out[k] = v
    return SignWeights(out, scales, shapes)


def dequantize_tensor(bits: torch.Tensor, scales: torch.Tensor, shape) -> torch.Tensor:
    """The fp32 tensor of ``shape`` whose element ``e`` is ``-scales[e // 256]`` where bit ``e`` is set and
    ``+scales[e // 256]`` where it is not; pad bits are ignored."""
    n = math.prod(shape)
    shifts = torch.arange(8, dtype=torch.int32, device=bits.device)
    neg = ((bits.view(-1, 1).to(torch.int32) >> shifts) & 1).reshape(-1)[:n].bool()
    mag = scales.repeat_interleave(BLOCK)[:n]
    return torch.where(neg, -mag, mag).reshape(tuple(shape))


def dequantize(w: SignWeights) -> dict:
    """``{key: fp32 tensor}`` for the compressed keys of ``w``; every other key as it is."""
    return collections.OrderedDict(
        (k, dequantize_tensor(v, w.scales[k], w.shapes[k]) if k in w.scales else v) for k, v in w.items())


def apply_(model: dict, msg) -> dict:
    """The trainer's side of the sign downlink (``egress.MessageEncoder(sign=True)``): ``msg`` applied to
    ``model`` in place.  A compressed key of a :class:`SignWeights` is the change since the last message:
    ``model[k] += dequantize_tensor(...)``, one fp32 add per element.  Every other key, and every key of a
    plain dict, is copied over.  Applied to every message in order, a compressed key holds bit for bit the
    encoder's base.  Returns ``model``."""
    sent = msg.scales if isinstance(msg, SignWeights) else {}
    for k, v in msg.items():
        if k in sent:
            model[k] += dequantize_tensor(v, sent[k], msg.shapes[k]).to(model[k].device)
        elif isinstance(v, torch.Tensor) and isinstance(model.get(k), torch.Tensor) and model[k].shape == v.shape \
                and model[k].dtype == v.dtype:
            model[k].copy_(v)
        else:
            model[k] = v.clone() if isinstance(v, torch.Tensor) else v
    return model


class ErrorFeedback:
    """The trainer's residual (EF-signSGD): :meth:`compress` sends ``delta + residual`` and keeps, per
    compressed key, ``residual = (delta + residual) - dequantize(sent)`` in fp32."""

    def __init__(self, min_numel: int = 0):
        self.min_numel, self.residual = min_numel, {}

    def compress(self, delta) -> SignWeights:
        full = collections.OrderedDict(
            (k, v.float() + self.residual[k] if k in self.residual else v) for k, v in delta.items())
        sent = compress(full, self.min_numel)
        dense = dequantize(sent)
        self.residual = {k: full[k].float() - dense[k] for k in sent.scales}
        return sent

    def reset(self) -> None:
        self.residual = {}
