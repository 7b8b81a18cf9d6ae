"""The noise generator of ``flame_noise_fill`` restated in numpy (helper of the noise tests; a plain module).

DESIGN.md §2, "the noise contract": a pure function of ``(seed, round, stream, index)``.

* Bits: Philox4x32-10 (Salmon et al., SC'11).  Key ``(seed & 0xffffffff, seed >> 32)``; counter
  ``(b & 0xffffffff, b >> 32, stream, round)`` with ``b = g >> 2``, ``g`` the element's global index in
  its key.  The four output words serve elements ``4b .. 4b+3``.
* Uniforms: ``(x0, x1)`` give elements ``4b`` and ``4b+1``, ``(x2, x3)`` give ``4b+2`` and ``4b+3``.
  ``u1 = RNE_f32(2 x + 1) * 2^-33`` in (0, 1]; the angle is ``2 pi k / 2^24`` with ``k = x' >> 8``.
* Transform: Box-Muller, ``r = sqrt(-2 ln u1)``, ``z_even = r cos``, ``z_odd = r sin``.

Every floating-point step below is ONE numpy ``float32`` operation (numpy never fuses a product
into a sum), in the order ``noise_pair`` of ``flame_amd/csrc/fedagg.hip`` performs them with
``__fmul_rn`` / ``__fadd_rn`` / ``__fdiv_rn`` and a correctly rounded root, so the device result is
this module's bit for bit.  The constants are written as the same hexadecimal literals.
"""
import math

import numpy as np

F = np.float32
U64 = np.uint64
MASK = U64(0xFFFFFFFF)
M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = U64(0x9E3779B9), U64(0xBB67AE85)


def _c(hexstr):
    v = float.fromhex(hexstr)
    assert float(F(v)) == v, hexstr         # exactly an fp32 value
    return F(v)


SQRT2 = _c("0x1.6a09e6p+0")
LN2_HI, LN2_LO = _c("0x1.62e4p-1"), _c("0x1.7f7d1cp-20")      # ln 2 = HI + LO; e * HI is exact for |e| <= 2^9
LOG = [_c(h) for h in ("0x1.555556p-2", "0x1.99999ap-3", "0x1.24924ap-3", "0x1.c71c72p-4", "0x1.745d18p-4")]   # 1/3 .. 1/11
PI_2_23 = _c("0x1.921fb6p-22")                                 # pi / 2^23: one octant is 2^21 steps
SIN = [_c(h) for h in ("-0x1.555556p-3", "0x1.111112p-7", "-0x1.a01a02p-13", "0x1.71de3ap-19")]     # -1/3! .. 1/9!
COS = [_c(h) for h in ("-0x1p-1", "0x1.555556p-5", "-0x1.6c16c2p-10", "0x1.a01a02p-16", "-0x1.27e4fcp-22")]  # -1/2! .. -1/10!


def philox4x32_10(counter, key):
    """One Philox4x32-10 block per row: ``counter`` four and ``key`` two arrays (or ints) of 32-bit
    words; returns the four output words as uint64 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=U64)) & MASK for x in counter]
    k = [np.atleast_1d(np.asarray(x, dtype=U64)) & MASK for x in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> U64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def blocks(seed, rnd, stream, b):
    """The output words of blocks ``b`` (uint64 array) of key ``stream`` in round ``rnd``."""
    b = np.asarray(b, dtype=U64)
    full = np.full(b.shape, 0, dtype=U64)
    return philox4x32_10((b & MASK, b >> U64(32), full + U64(stream & 0xFFFFFFFF), full + U64(rnd & 0xFFFFFFFF)),
                         (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def uniform_of(x):
    """``u1 = RNE_f32(2 x + 1) * 2^-33``: the 33-bit odd integer as an exact high part (16 bits, scaled)
    plus an exact low part (17 bits), so the one rounding is the add's."""
    v = np.asarray(x, dtype=U64) * U64(2) + U64(1)
    hi = (v >> U64(17)).astype(F)
    lo = (v & U64(0x1FFFF)).astype(F)
    return (hi * F(131072.0) + lo) * F(2.0 ** -33)


def neg2ln(u):
    """``-2 ln u`` for fp32 ``u`` in (0, 1]."""
    bits = np.ascontiguousarray(u, dtype=F).view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int32) - np.int32(127)
    m = ((bits & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(F)
    big = m > SQRT2
    m = np.where(big, m * F(0.5), m)
    e = e + big.astype(np.int32)
    f = m - F(1.0)
    s = f / (f + F(2.0))
    z = s * s
    p = LOG[4]
    for cst in (LOG[3], LOG[2], LOG[1], LOG[0]):
        p = p * z + cst
    p = p * z
    t = s + s
    lg = t + t * p                      # ln m = 2 atanh(s)
    ef = e.astype(F)
    ln = ef * LN2_HI + (lg + ef * LN2_LO)
    return F(-2.0) * ln


def sincos(k):
    """``(cos, sin)`` of ``2 pi k / 2^24`` for 24-bit ``k``: octant reduction on the integer, then the
    polynomials on [0, pi/4]."""
    k = np.asarray(k, dtype=np.uint32)
    o = k >> np.uint32(21)
    j = k & np.uint32(0x1FFFFF)
    jj = np.where(o & np.uint32(1), np.uint32(0x200000) - j, j)
    phi = jj.astype(F) * PI_2_23
    z = phi * phi
    ps = SIN[3]
    for cst in (SIN[2], SIN[1], SIN[0]):
        ps = ps * z + cst
    s = phi + (phi * z) * ps
    pc = COS[4]
    for cst in (COS[3], COS[2], COS[1], COS[0]):
        pc = pc * z + cst
    c = F(1.0) + z * pc
    swap = ((o + np.uint32(1)) >> np.uint32(1)) & np.uint32(1)
    cneg = ((o + np.uint32(2)) >> np.uint32(2)) & np.uint32(1)
    sneg = o >> np.uint32(2)
    co = np.where(swap, s, c)
    si = np.where(swap, c, s)
    return np.where(cneg, -co, co), np.where(sneg, -si, si)


def pair(xu, xk):
    """Two unit normals from two Philox words: ``(z_even, z_odd)``."""
    r = np.sqrt(neg2ln(uniform_of(xu)))
    co, si = sincos((np.asarray(xk, dtype=U64) >> U64(8)).astype(np.uint32))
    return r * co, r * si


def block_normals(seed, rnd, stream, b):
    """``z[len(b), 4]``: the four fp32 unit normals of each block."""
    x0, x1, x2, x3 = blocks(seed, rnd, stream, b)
    z = np.empty((len(x0), 4), dtype=F)
    z[:, 0], z[:, 1] = pair(x0, x1)
    z[:, 2], z[:, 3] = pair(x2, x3)
    return z


def unit_normals(seed, rnd, stream, start, n):
    """fp32 ``z[g]`` for ``g`` in ``[start, start + n)`` of key ``stream``."""
    if n <= 0:
        return np.empty(0, dtype=F)
    b0, b1 = start >> 2, (start + n - 1) >> 2
    b = np.arange(b1 - b0 + 1, dtype=U64) + U64(b0)
    z = block_normals(seed, rnd, stream, b).reshape(-1)
    off = start - 4 * b0
    return np.ascontiguousarray(z[off:off + n])


def bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even (a NaN stays a NaN)."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, np.uint16(0x7FC0), r)


def fill(dtype, seed, rnd, stream, start, n, std):
    """``noise[e] = round_dtype(z[start + e] * std)`` as a numpy array: ``"f32"`` float32, ``"f16"``
    float16, ``"f64"`` float64, ``"bf16"`` the uint16 bit patterns.  f32 / bf16 / f16 take ``std``
    rounded to fp32 and one fp32 multiply (16-bit: then one RNE rounding); f64 widens ``z`` and takes
    one fp64 multiply by the Python float."""
    z = unit_normals(seed, rnd, stream, start, n)
    if dtype == "f64":
        return z.astype(np.float64) * np.float64(std)
    with np.errstate(over="ignore"):
        x = z * F(std)
        if dtype == "f32":
            return x
        if dtype == "f16":
            return x.astype(np.float16)
    if dtype == "bf16":
        return bf16_bits(x)
    raise ValueError(dtype)


NAMES = {"torch.float32": "f32", "torch.bfloat16": "bf16", "torch.float16": "f16", "torch.float64": "f64"}


def fill_torch(like, seed, rnd, stream, start, std, n=None):
    """:func:`fill` as a CPU torch tensor of ``like``'s dtype (and shape, unless ``n`` is given)."""
    import torch
    name = NAMES[str(like.dtype)]
    a = fill(name, seed, rnd, stream, start, like.numel() if n is None else n, std)
    if name == "bf16":
        t = torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    else:
        t = torch.from_numpy(np.ascontiguousarray(a))
    return t.reshape(like.shape) if n is None else t


def std_of(noise_factor, rates):
    """``s * sqrt(fsum(rate^2))`` in Python floats (``flame_amd/optimizer/noise.py`` states the same)."""
    return float(noise_factor) * math.sqrt(math.fsum(float(r) * float(r) for r in rates))
