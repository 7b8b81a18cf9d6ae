"""Low-rank updates: the trainer-side format of the factor-pair uplink (torch only, no native code).

A low-rank update holds a factored key ``W [m, n]`` as a left factor ``U [m, r]`` and a right factor
``V [r, n]``: a LoRA adapter pair, or a PowerSGD-style factorisation of a delta.  At rank 16 a
4,096 x 4,096 key is 0.8 % of its fp32 bytes.

    from flame_amd import lowrank
    sent = lowrank.compress(delta, rank=16)                 # trainer: a LowRankWeights, sent as the update
    dense = lowrank.densify(sent)                           # the update's value, U @ V
    residual = {k: delta[k] - dense[k] for k in delta}      # error feedback: residual = delta - densify(sent)

A LoRA trainer sends its adapters as they are, its scaling folded into the left factor:

    sent = lowrank.LowRankWeights({k: lora_B * (alpha / r)}, right={k: lora_A}, shapes={k: W.shape})

The contract ("the low-rank contract"): the aggregate is the EXACT one,
``W += sum_c rate_c * U_c @ V_c`` (FLoRA), not the product of the averaged factors that a plain FedAvg
over adapter keys computes.  Per element, ``out[i,j] = in[i,j] + sum_c sum_q f32(U_c[i,q] * rate_c) *
V_c[q,j]``, accumulated in fp32 on the matrix cores; clients may hold different ranks, 0 included.  The
aggregator's kernel is ``flame_agg_reduce_lowrank``.
"""
from __future__ import annotations

import collections
import math

import torch

FACTORED_FROM = (torch.float32, torch.bfloat16, torch.float16)
FACTOR_DTYPES = (torch.float32, torch.bfloat16)


def matrix_shape(shape) -> tuple:
    """``(m, n)`` of a key of logical shape ``shape`` (two dimensions or more): ``(shape[0], prod(shape[1:]))``."""
    return int(shape[0]), math.prod(int(d) for d in shape[1:])


class LowRankWeights(dict):
    """One trainer's update.  A factored key holds its left factor ``U``, a contiguous ``[m, r]`` tensor;
    every other key the plain tensor it always held.  ``right``: ``{key: V}``, a contiguous ``[r, n]``
    tensor of ``U``'s dtype (fp32 or bf16).  ``shapes``: ``{key: logical shape}``; a key of more than two
    dimensions is factored as ``(shape[0], prod(shape[1:]))``."""

    def __init__(self, weights=(), right=None, shapes=None):
        super().__init__(weights)
        self.right = dict(right) if right is not None else {}
        self.shapes = {k: tuple(v) for k, v in shapes.items()} if shapes is not None else {}

    def __reduce__(self):
        return (LowRankWeights, (dict(self), self.right, self.shapes))

    def _map(self, f):
        return LowRankWeights(((k, f(v) if isinstance(v, torch.Tensor) else v) for k, v in self.items()),
                              {k: f(v) for k, v in self.right.items()}, self.shapes)

    def to(self, device, non_blocking: bool = False):
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def pin_memory(self):
        return self._map(lambda t: t.pin_memory())


def compress(weights, rank: int, min_numel: int = 0, dtype=torch.float32) -> LowRankWeights:
    """``weights`` (a state_dict-style mapping) as a :class:`LowRankWeights`: every fp32 / bf16 / f16 key of
    at least two dimensions and at least ``min_numel`` elements is replaced by its truncated SVD
    (``torch.linalg.svd(full_matrices=False)`` of the fp32 matrix), ``U = U_r * S_r`` and ``V = Vh_r`` of rank
    ``min(rank, m, n)``, both cast to ``dtype`` (fp32 or bf16); every other key passes through unchanged.
    Runs where the tensors live."""
    if isinstance(rank, bool) or not isinstance(rank, int) or rank < 1:
        raise ValueError(f"flame_amd.lowrank.compress: rank {rank!r} is not a positive integer")
    if dtype not in FACTOR_DTYPES:
        raise ValueError(f"flame_amd.lowrank.compress: factor dtype {dtype} is not torch.float32 or torch.bfloat16")
    out, right, shapes = collections.OrderedDict(), {}, {}
    for k, v in weights.items():
        if isinstance(v, torch.Tensor) and v.dtype in FACTORED_FROM and v.dim() >= 2 and v.numel() >= max(min_numel, 1):
            m, n = matrix_shape(v.shape)
            u, s, vh = torch.linalg.svd(v.detach().reshape(m, n).to(torch.float32), full_matrices=False)
            r = min(rank, m, n)
            out[k] = (u[:, :r] * s[:r]).to(dtype).contiguous()
            right[k], shapes[k] = vh[:r].to(dtype).contiguous(), tuple(v.shape)
        else:
            out[k] = v
    return LowRankWeights(out, right, shapes)


def apply_(model: dict, msg) -> dict:
    """The trainer's side of the low-rank downlink (``egress.MessageEncoder(lowrank=)``): ``msg`` applied to
    ``model`` in place.  A factored key of a :class:`LowRankWeights` is the change since the last message:
    ``model[k] += (U @ V).view(shape)``, the product in fp32 where the model lives.  Every other key, and every
    key of a plain dict, is copied over.  The encoder's base took the same product from the matrix cores, which
    round in another order: the two differ by at most the any-order fp32 bound of a length-r dot product per
    message, ``gamma_r |U| |V|``, and the differences add up until the next dense message.  Returns ``model``."""
    right = msg.right if isinstance(msg, LowRankWeights) else {}
    for k, v in msg.items():
        if k in right:
            dev = model[k].device
            model[k] += (v.to(dev, torch.float32) @ right[k].to(dev, torch.float32)).view(model[k].shape)
        elif isinstance(v, torch.Tensor) and isinstance(model.get(k), torch.Tensor) and model[k].shape == v.shape \
                and model[k].dtype == v.dtype:
            model[k].copy_(v)
        else:
            model[k] = v.clone() if isinstance(v, torch.Tensor) else v
    return model


def densify(w: LowRankWeights) -> dict:
    """``{key: fp32 U @ V in the key's logical shape}`` for the factored keys of ``w``; every other key as it is."""
    out = collections.OrderedDict()
    for k, v in w.items():
        if k in w.right:
            out[k] = (v.to(torch.float32) @ w.right[k].to(torch.float32)).reshape(w.shapes[k])
        else:
            out[k] = v
    return out
