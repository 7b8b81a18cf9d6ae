"""The top-k selection's reference ("the top-k selection"), a few lines of numpy: the k largest keys
``bits(f32(x)) & 0x7FFFFFFF``, among equal keys the lowest indices, sorted by index."""
import numpy as np


def f32(t):
    """A torch tensor's elements as a flat numpy fp32 array (a 16-bit dtype widened exactly)."""
    return t.detach().cpu().reshape(-1).float().numpy()


def topk(x, k, base=None):
    """``(indices int32 [k], values fp32 [k], the base afterwards or None)`` for the fp32 array ``x``."""
    with np.errstate(all="ignore"):
        d = x if base is None else (x - base).astype(np.float32)
    key = d.view(np.uint32) & np.uint32(0x7FFFFFFF)
    idx = np.sort(np.lexsort((np.arange(d.size), -key.astype(np.int64)))[:k])
    if base is not None:
        base = base.copy()
        with np.errstate(all="ignore"):
            base[idx] = (base[idx] + d[idx]).astype(np.float32)
    return idx.astype(np.int32), d[idx], base
