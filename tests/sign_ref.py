"""The sign contract as a sequential fp32 loop in numpy: per client in order, acc = acc + (+-s) * rate32."""
import numpy as np


def accumulate(base, ups, rates):
    """``base``: fp32 array; ``ups``: one ``(bits uint8, scales fp32)`` per client; the fp32 aggregate."""
    acc, n = base.astype(np.float32).reshape(-1), base.size
    with np.errstate(all="ignore"):
        for (bits, scales), r in zip(ups, rates):
            neg = np.unpackbits(bits, bitorder="little")[:n].astype(bool)       # pad bits dropped
            s = np.repeat(scales.astype(np.float32), 256)[:n]
            acc = acc + np.where(neg, -s, s) * np.float32(r)
    return acc.reshape(base.shape)
