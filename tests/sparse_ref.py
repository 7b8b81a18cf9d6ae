"""The sparse contract in numpy.  A plain module, no tests."""
import numpy as np


def accumulate(base, updates, rates, scales=None):
    """``base`` (fp32, any shape) after ``updates``, ``[(int32 indices, fp32 values)]`` in client order; a new array."""
    acc = np.array(base, dtype=np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        for c, (idx, val) in enumerate(updates):
            t = np.asarray(val, dtype=np.float32)
            if scales is not None:
                t = (t * np.float32(scales[c])).astype(np.float32)
            t = (t * np.float32(rates[c])).astype(np.float32)
            acc[idx] = (acc[np.asarray(idx)] + t).astype(np.float32)        # a client's indices are unique
    return acc.reshape(np.shape(base))
