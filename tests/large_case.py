"""Shared pieces of the maximum-size tests (tests/test_gpu_large.py, tests/test_gpu_large_kernels.py):
one state_dict key whose element index crosses 2^31 (and 2^32), filled by the counter generator on
the device and checked at a sample of its elements.  A plain module, no tests.

* ``P32 = 2^31 + 4099``: fp32 / fp64 keys.  Crosses the signed 32-bit element index and, in fp32,
  every byte offset past 4 GiB.
* ``P16 = 2^32 + 70,001``: 1- and 2-byte keys (a bf16 tensor of P16 elements has the bytes of an
  fp32 one of P32).  Crosses the signed AND the unsigned 32-bit element index and byte offsets 2^32
  and 2^33; the tail past 2^32 is 34 whole bf16 chunks plus 369 elements.

The sample (:func:`index`) holds the boundaries, every element at or past 2^32 and 20,000 seeded
random indices: uniform sampling alone puts about 10 of 20,000 samples past 2^32, so that tail is
taken whole.  The reference's inputs never come back from the device: :func:`host_synth` restates
the generator on the host, and every case asserts that the device holds those bits.
"""
import numpy as np
import pytest
import torch

DEV = "cuda:0"
P32 = (1 << 31) + 4099          # a ragged tail after the 2^31st element
P16 = (1 << 32) + 70_001        # a ragged tail after the 2^32nd element


def _need(gb):
    free, _ = torch.cuda.mem_get_info()
    if free < gb * 1e9:
        pytest.skip(f"needs {gb} GB of HBM, {free / 1e9:.1f} GB free")


def _synth(P, seed, stream, sigma, dtype=torch.float32):
    """``P`` elements of the counter generator on the device (fp64: the fp32 values widened)."""
    from flame_amd import engine
    if dtype == torch.float64:
        return _synth(P, seed, stream, sigma).double()
    t = torch.empty(P, dtype=dtype, device=DEV)
    engine.synth_fill_(t, seed, stream, 0, sigma)
    return t


def host_synth(seed, stream, idx, sigma, dtype=torch.float32):
    """The generator's values at the element indices ``idx`` (an int64 tensor), restated on the host
    (flame_amd.synth): what :func:`_synth` must hold there, bit for bit."""
    from flame_amd import synth
    x = synth.synth_f32(seed, stream, idx.numpy(), sigma)
    if dtype == torch.float32:
        return torch.from_numpy(x)
    if dtype == torch.float64:
        return torch.from_numpy(x.astype(np.float64))
    if dtype == torch.float16:
        return torch.from_numpy(x.astype(np.float16))
    assert dtype == torch.bfloat16, dtype
    return torch.from_numpy(synth.f32_to_bf16_bits(x).view(np.int16)).view(torch.bfloat16)


def boundaries(P):
    """The element indices where an index can go wrong: 0, 2^30, 2^31, 2^32 (when ``P`` is past it),
    the chunk seams next to those (chunks of 1,024 to 4,096 elements), the start of the ragged tail
    and 2,048 before the end."""
    top = 1 << 32 if P > 1 << 32 else 1 << 31
    b = [0, 1 << 30, (1 << 31) - 2048, 1 << 31]
    if P > 1 << 32:
        b += [(1 << 31) + 2048, (1 << 32) - 4096, (1 << 32) - 2048, (1 << 32) - 1024, 1 << 32]
    return b + [top, P - 2048]


def index(P):
    """The sample set: three elements either side of every :func:`boundaries` entry, the first two
    chunk seams, ``P - 1``, every element at or past 2^32, and 20,000 seeded random indices."""
    edges = []
    for b in boundaries(P):
        edges += list(range(max(0, b - 3), min(P, b + 3)))
    edges += [1023, 1024, 1025, 2047, 2048, P - 1]
    rand = np.random.default_rng(0).integers(0, P, 20_000)
    parts = [np.array(edges), rand]
    if P > 1 << 32:
        parts.append(np.arange(1 << 32, P))
    return torch.from_numpy(np.unique(np.concatenate(parts)).astype(np.int64))


def _at(t, idx):
    return t.index_select(0, idx.to(t.device)).cpu()


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def pinned(label, t, idx, want):
    """``t`` holds ``want`` at ``idx`` bit for bit (the device generator against the host's); returns
    ``want``, the reference's input."""
    got = _at(t, idx)
    assert got.dtype == want.dtype, (label, got.dtype, want.dtype)
    wide = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    bad = (got.view(wide) != want.view(wide)).nonzero().flatten()
    assert bad.numel() == 0, (f"{label}: the device generator differs from flame_amd.synth at {bad.numel()} of "
                              f"{idx.numel()} samples, first at element {int(idx[bad[0]])}")
    return want


# A case's inputs: stream 0 is the base (or model), stream 1 + i update i.  One seed per case, shared
# with tests/test_large_case_host.py, which checks that these very inputs would show a wrapped index.
UP_SIGMA = 1e-2
SEED = {"scaled": 21, "mixed": 22, "mx": 23, "trimmed": 24, "select": 25, "stats": 26, "scale_add": 28,
        "elementwise": 29, "feddyn": 30, "chain": 31, "f64": 32}
RATES = [3 / 19, 5 / 19]            # two clients
ROBUST_BASE_SIGMA = 1e-2            # the median of 3 over a base whose bf16 ulp does not swallow it


def case_host(seed, idx, n, base_sigma, base_dtype, up_dtype):
    """``(base, [update 0 .. n-1])`` at ``idx`` from the host generator."""
    return (host_synth(seed, 0, idx, base_sigma, base_dtype),
            [host_synth(seed, 1 + i, idx, UP_SIGMA, up_dtype) for i in range(n)])


def case_dev(P, seed, idx, n, base_sigma, base_dtype, up_dtype):
    """The same case on the device, each tensor pinned against :func:`case_host` at ``idx``:
    ``(base, updates, base samples, update samples)``."""
    b_s, u_s = case_host(seed, idx, n, base_sigma, base_dtype, up_dtype)
    base = _synth(P, seed, 0, base_sigma, base_dtype)
    pinned(f"seed {seed} base", base, idx, b_s)
    ups = []
    for i in range(n):
        ups.append(_synth(P, seed, 1 + i, UP_SIGMA, up_dtype))
        pinned(f"seed {seed} update {i}", ups[i], idx, u_s[i])
    return base, ups, b_s, u_s


# Reductions along an update cannot be sampled: the sums are made exact instead.
DENSE_SIGMA, DENSE_MAX = 3.0, 8
SENTINEL_VALUES = (1, 2, 4, 8, 16, 32)


def integer_valued(t):
    """The dense recipe, in place: every value an integer of [-8, 8], exact in bf16, so that every
    square, product and partial sum over P16 elements stays below 64 * P16 < 2^39 and the fp64
    result is the exact integer in any summation order."""
    return t.round_().clamp_(-DENSE_MAX, DENSE_MAX)


def sentinels(P):
    """Six positions either side of the 32-bit boundaries; the sparse updates hold
    ``SENTINEL_VALUES`` there, so ``sumsq`` = sum(4**j) and a missed or doubled read shows in its
    binary digits."""
    return [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, P - 1]


class Launches:
    """Names of the native launches made inside the block (engine._recorders)."""

    def __enter__(self):
        from flame_amd import engine
        self.events = []
        engine._recorders.append(self.events)
        return self

    def __exit__(self, *exc):
        from flame_amd import engine
        engine._recorders.remove(self.events)
        self.names = [ev[0] for ev in self.events]
        self.bytes = {ev[0]: ev[3] for ev in self.events}
        return False

    def count(self, name):
        return sum(1 for n in self.names if n == name)

    def elementwise(self):
        return sum(1 for n in self.names if n.startswith("flame_elementwise"))
