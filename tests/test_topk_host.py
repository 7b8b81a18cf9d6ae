"""The top-k selection's host side: the reference of the GPU tests, sparse.apply_, the encoder's refusals and the
plan.  No GPU."""
import numpy as np
import pytest
import torch

import topk_ref as R
from flame_amd import _native as N
from flame_amd import egress, engine, sparse


def test_reference_agrees_with_sparse_topk_without_ties():
    x = torch.randperm(5000, generator=torch.Generator().manual_seed(2)).float().add(1).view(50, 100)
    x[:, ::2] *= -1                                                    # distinct magnitudes, both signs
    w = sparse.topk({"k": x}, 0.013)
    idx, val, _ = R.topk(R.f32(x), 65)
    assert np.array_equal(idx, w.indices["k"].numpy()) and np.array_equal(val, w["k"].numpy())


def test_apply_inverts_densify():
    model = {"w": torch.arange(12.0).view(3, 4), "b": torch.zeros(2), "steps": torch.tensor([1])}
    before = model["w"].clone()
    msg = sparse.SparseWeights({"w": torch.tensor([0.5, -2.0, 8.0]), "b": torch.ones(2), "steps": torch.tensor([5])},
                               {"w": torch.tensor([1, 6, 11], dtype=torch.int32)}, {"w": (3, 4)})
    assert sparse.apply_(model, msg) is model
    assert torch.equal(model["w"], before + sparse.densify(msg)["w"]) and torch.equal(model["b"], torch.ones(2))
    assert torch.equal(model["steps"], torch.tensor([5]))
    sparse.apply_(model, {"w": before, "new": torch.ones(1)})            # a plain dict: every key copied over
    assert torch.equal(model["w"], before) and torch.equal(model["new"], torch.ones(1))


@pytest.mark.parametrize("kwargs", [{"mx": "e4m3", "sparse": 0.01}, {"sparse": 0}, {"sparse": 1.5}])
def test_encoder_refusals(kwargs):
    with pytest.raises(ValueError):
        egress.MessageEncoder(pin=False, **kwargs)


def test_plan_lays_every_segment_on_a_chunk_start():
    C = int(N.lib().flame_topk_chunk_elems())
    numels, ks = [1, C, C + 1, 3 * C - 1], [1, 7, C + 1, 40]
    segs = [engine.Seg(n, out=0x1000 * i, inp=0x2000 * i + (4 if i == 2 else 0), cur_out=0x3000 * i, m=0x4000 * i)
            for i, n in enumerate(numels, 1)]
    meta, n_chunks = engine.plan_topk(segs, ks)
    head = meta[:4 * engine.SEG_WORDS].reshape(4, engine.SEG_WORDS)
    assert n_chunks == 1 + 1 + 2 + 3 and head[:, 7].tolist() == [0, 1, 2, 4] and head[:, 6].tolist() == numels
    assert head[:, 8].tolist() == [0, N.FLAME_SEG_UNALIGNED, 0, 0] and meta[4 * engine.SEG_WORDS:].tolist() == ks
    assert head[2, [0, 1, 3, 4]].tolist() == [0x3000, 0x6000, 0x9000, 0xC000]       # out, in, cur_out, m
    for bad in ([0, 7, 1, 1], [1, C + 1, 1, 1]):
        with pytest.raises(ValueError):
            engine.plan_topk(segs, bad)
