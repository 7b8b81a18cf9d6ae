"""The sparse launches over three fp32 keys, each under 2^31 elements, whose chunks together pass 2^32 elements (a chunk's
global offset or bounds row in 32 bits would wrap); entries around the segment ends, 2^30 and the crossing, sampled bitwise."""
import numpy as np
import pytest
import torch

import large_case as LC
import scenarios as S
import sparse_ref
from large_case import DEV, Launches, _at, _free, _need

pytestmark = [pytest.mark.gpu]
SIZES, SEED = {"p": (1 << 31) - 4097, "q": (1 << 31) - 4097, "r": (1 << 20) + 3}, 33      # 2^32 falls 8,194 elements into r


def test_sparse_chunks_past_2_32_elements():
    from flame_amd import engine, sparse
    _need(4 * sum(SIZES.values()) / 1e9 + 3)
    rng, agg, want, cands = np.random.default_rng(SEED), {}, {}, {}
    ups = [sparse.SparseWeights(shapes={k: (m,) for k, m in SIZES.items()}) for _ in range(2)]
    for stream, (k, m) in enumerate(SIZES.items()):
        spots = [0, 1 << 30, m - 1200] + ([(1 << 32) - SIZES["p"] - SIZES["q"] - 600] if k == "r" else [])
        cand = np.unique(np.concatenate([np.arange(s, min(m, s + 1200)) for s in spots]))
        cands[k] = torch.from_numpy(cand)
        agg[k] = LC._synth(m, SEED, stream, 1.0)
        b_s = LC.pinned(f"sparse base {k}", agg[k], cands[k], LC.host_synth(SEED, stream, cands[k], 1.0))
        sent = []
        for w in ups:
            idx = np.sort(rng.choice(cand, int(0.6 * cand.size), replace=False))
            val = (rng.standard_normal(idx.size) * 1e-2).astype(np.float32)
            w[k], w.indices[k] = torch.from_numpy(val).to(DEV), torch.from_numpy(idx.astype(np.int32)).to(DEV)
            sent.append((np.searchsorted(cand, idx), val))      # positions in the sample
        want[k] = torch.from_numpy(sparse_ref.accumulate(b_s.numpy(), sent, LC.RATES))
    with Launches() as ln:
        engine.accumulate(agg, list(zip(ups, LC.RATES)))
    assert ln.names == ["flame_sparse_index", "flame_agg_reduce_sparse"], ln.names
    S.same_bits("large sparse", {k: _at(agg[k], cands[k]) for k in SIZES}, want)
    agg.clear(), ups.clear(), _free()
