"""Top-k sparse updates: the trainer-side format of the index/value uplink (torch only, no native code).

A sparse update holds a sparsified float key as its ``nnz`` largest-magnitude elements: one fp32 value
and one int32 flat C-order element index each, the indices strictly ascending.  At 1 % density that is
0.08 bytes per parameter, against 4 for fp32 and 0.53 for MXFP4.

    from flame_amd import sparse
    sent = sparse.topk(delta, ratio=0.01)                   # trainer: a SparseWeights, sent as the update
    dense = sparse.densify(sent)                            # the update's value where something was sent
    residual = {k: delta[k] - dense[k] for k in delta}      # error feedback: residual = delta - densify(sent)

The contract ("the sparse contract"): an absent element contributes NOTHING to the
aggregate, not a zero.  Per element ``e`` of an fp32 key, starting from ``acc = in[e]``, the clients that
hold ``e`` are taken in cache order, ``acc = f32(acc + f32(v * rate_i))`` (with clip scales
``f32(f32(v * scale_i) * rate_i)``), no FMA, denormals kept.  That is the dense fp32 round over
``densify(update)`` bit for bit, except that an untouched ``-0.0`` stays ``-0.0``.  The aggregator's
kernels are ``flame_sparse_index`` and ``flame_agg_reduce_sparse``.
"""
from __future__ import annotations

import collections
import math

import torch

SPARSIFIED_FROM = (torch.float32, torch.bfloat16, torch.float16)
INDEX_LIMIT = 2 ** 31       # int32 indices address elements [0, 2^31)


class SparseWeights(dict):
    """One trainer's update.  A sparsified key holds its values, a 1-D fp32 tensor of ``nnz`` elements;
    every other key the plain tensor it always held.  ``indices``: ``{key: int32 [nnz]}``, the flat
    C-order element indices, strictly ascending.  ``shapes``: ``{key: logical shape}``."""

    def __init__(self, weights=(), indices=None, shapes=None):
        super().__init__(weights)
        self.indices = dict(indices) if indices is not None else {}
        self.shapes = {k: tuple(v) for k, v in shapes.items()} if shapes is not None else {}

    def __reduce__(self):
        return (SparseWeights, (dict(self), self.indices, self.shapes))

    def _map(self, f):
        return SparseWeights(((k, f(v) if isinstance(v, torch.Tensor) else v) for k, v in self.items()),
                             {k: f(i) for k, i in self.indices.items()}, self.shapes)

    def to(self, device, non_blocking: bool = False):
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def pin_memory(self):
        return self._map(lambda t: t.pin_memory())


def topk(weights, ratio: float = 0.01, min_numel: int = 0) -> SparseWeights:
    """``weights`` (a state_dict-style mapping) as a :class:`SparseWeights`: fp32 / bf16 / f16 keys of at
    least ``min_numel`` elements keep their ``k = max(1, ceil(ratio * numel))`` largest ``|x|`` (values
    widened to fp32, indices sorted); every other key passes through unchanged.  A key of 2^31 elements
    or more raises ValueError: int32 indices cannot address it.  Runs where the tensors live."""
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"flame_amd.sparse.topk: ratio {ratio!r} is not in (0, 1]")
    out, indices, shapes = collections.OrderedDict(), {}, {}
    for k, v in weights.items():
        if isinstance(v, torch.Tensor) and v.dtype in SPARSIFIED_FROM and v.numel() >= max(min_numel, 1):
            n = v.numel()
            if n >= INDEX_LIMIT:
                raise ValueError(f"flame_amd.sparse.topk: key {k!r} has {n} elements; int32 indices address fewer than 2^31")
            flat = v.detach().reshape(-1)
            idx = flat.abs().topk(min(n, max(1, math.ceil(ratio * n))), sorted=False).indices.sort().values
            out[k], indices[k], shapes[k] = flat[idx].to(torch.float32), idx.to(torch.int32), tuple(v.shape)
        else:
            out[k] = v
    return SparseWeights(out, indices, shapes)


def apply_(model: dict, msg) -> dict:
    """The trainer's side of the sparse downlink (``egress.MessageEncoder(sparse=)``): ``msg`` applied to
    ``model`` in place.  A sparsified key of a :class:`SparseWeights` is the change since the last message:
    ``flat[idx] = flat[idx] + v``, one fp32 add per sent element (the indices are unique).  Every other key,
    and every key of a plain dict, is copied over.  Applied to every message in order, a sparsified key holds
    bit for bit the encoder's base.  Returns ``model``."""
    sent = msg.indices if isinstance(msg, SparseWeights) else {}
    for k, v in msg.items():
        if k in sent:
            flat, idx = model[k].view(-1), sent[k].to(model[k].device).long()
            flat[idx] = flat[idx] + v.to(flat.device)
        elif isinstance(v, torch.Tensor) and isinstance(model.get(k), torch.Tensor) and model[k].shape == v.shape \
                and model[k].dtype == v.dtype:
            model[k].copy_(v)
        else:
            model[k] = v.clone() if isinstance(v, torch.Tensor) else v
    return model


def densify(w: SparseWeights) -> dict:
    """``{key: fp32 tensor}`` for the sparsified keys of ``w``, zeros where nothing was sent; every other
    key as it is."""
    out = collections.OrderedDict()
    for k, v in w.items():
        if k in w.indices:
            flat = torch.zeros(math.prod(w.shapes[k]), dtype=torch.float32, device=v.device)
            flat[w.indices[k].long()] = v
            out[k] = flat.reshape(w.shapes[k])
        else:
            out[k] = v
    return out
