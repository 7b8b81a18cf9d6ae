"""A numpy restatement of the MXFP8 format (OCP Microscaling v1.0) by integer bit manipulation:
decode of e4m3fn / e5m2 / e8m0 bytes, block quantisation and dequantisation.  Independent of torch's
float8 casts, of frexp / ldexp and of any floating-point multiply but the contract's own (one fp32
product per element in ``dequantize``)."""
import numpy as np

BLOCK = 32
# name -> (exponent bits, mantissa bits, bias, emax, byte of the largest finite magnitude)
FMT = {"e4m3": (4, 3, 7, 8, 0x7E), "e5m2": (5, 2, 15, 15, 0x7B)}


def _pow2(e):
    """2^e as fp32 from its bits, e an int array in [-149, 127]."""
    e = np.asarray(e, dtype=np.int64)
    bits = np.where(e >= -126, (e + 127) << 23, 1 << np.clip(e + 149, 0, 22))
    return bits.astype(np.uint32).view(np.float32)


def decode(byte, fmt):
    """fp32 value of each fp8 byte."""
    eb, mb, bias, _, _ = FMT[fmt]
    b = np.asarray(byte, dtype=np.uint8).astype(np.int64)
    sign, ex, man = b >> 7, (b >> mb) & ((1 << eb) - 1), b & ((1 << mb) - 1)
    top = (1 << eb) - 1
    if fmt == "e4m3":
        nan, inf = (ex == top) & (man == 7), np.zeros(b.shape, bool)
    else:
        nan, inf = (ex == top) & (man != 0), (ex == top) & (man == 0)
    # man * 2^(1 - bias - mb) for subnormals, (2^mb + man) * 2^(ex - bias - mb) otherwise: integers
    # below 2^(mb + 1) times a power of two, exact in fp32
    sig = np.where(ex == 0, man, man + (1 << mb)).astype(np.float32)
    val = sig * _pow2(np.where(ex == 0, 1, ex) - bias - mb)
    val = np.where(inf, np.float32(np.inf), val)
    val = np.where(sign == 1, -val, val).astype(np.float32)
    return np.where(nan, np.float32(np.nan), val).astype(np.float32)


def decode_e8m0(byte):
    b = np.asarray(byte, dtype=np.uint8).astype(np.int64)
    bits = np.where(b == 255, 0x7FC00000, np.where(b == 0, 0x00400000, b << 23))
    return bits.astype(np.uint32).view(np.float32)


def quantize(x, fmt):
    """(element bytes [n], scale bytes [ceil(n / 32)]) of the flat fp32 array ``x``."""
    eb, mb, bias, emax, top_byte = FMT[fmt]
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
    n = x.size
    nb = -(-n // BLOCK)
    u = np.zeros(nb * BLOCK, dtype=np.uint32)
    u[:n] = x.view(np.uint32)
    u = u.reshape(nb, BLOCK).astype(np.int64)
    mag = u & 0x7FFFFFFF
    finite = mag < 0x7F800000
    amax = np.where(finite, mag, 0).max(axis=1)               # bits order as magnitudes do
    ex = amax >> 23
    # floor(log2 amax): normal from the exponent field, subnormal from the top set bit of the mantissa
    top_bit = np.floor(np.log2(np.maximum(amax & 0x7FFFFF, 1).astype(np.float64))).astype(np.int64)    # exact below 2^23
    fl = np.where(ex > 0, ex - 127, top_bit - 149)
    e = np.clip(fl - emax, -127, 127)
    e = np.where(amax == 0, 0, e)
    scale_byte = (e + 127).astype(np.uint8)
    # x * 2^-e in exact integer terms: shift the fp32 exponent; renormalise subnormals first
    sign = (u >> 31) & 1
    exf, man = mag >> 23, mag & 0x7FFFFF
    sig = np.where(exf == 0, man, man | 0x800000)
    e2 = np.where(exf == 0, -126, exf - 127) - e[:, None]      # value = sig * 2^(e2 - 23)
    out = _encode_sig(sig, e2, fmt)
    is_nan = mag > 0x7F800000
    is_inf = mag == 0x7F800000
    out = np.where(is_inf, top_byte, out)
    out = np.where(is_nan, 0x7F, out)               # a NaN in both formats (e4m3fn's only one)
    out = (out | (sign << 7)).astype(np.uint8)
    return out.reshape(-1)[:n], scale_byte


def _encode_sig(sig, e2, fmt):
    """The fp8 magnitude byte (sign clear) nearest-even to sig * 2^(e2 - 23), sig < 2^24, any integer
    e2, saturating at the largest finite value; integer arithmetic only."""
    eb, mb, bias, _, top_byte = FMT[fmt]
    sig = np.asarray(sig, dtype=np.int64)
    e2 = np.asarray(e2, dtype=np.int64)
    # normalise so that a nonzero sig has bit 23 set (a subnormal fp32 input)
    nz = sig > 0
    lead = np.floor(np.log2(np.maximum(sig, 1).astype(np.float64))).astype(np.int64)
    up = np.where(nz, 23 - lead, 0)
    sig = sig << up
    e2 = e2 - up
    q = np.maximum(e2 - mb, 1 - bias - mb)
    shift = np.clip(q - (e2 - 23), 0, 62)
    keep = sig >> shift
    rem = sig & ((np.int64(1) << shift) - 1)
    half = np.where(shift > 0, np.int64(1) << np.maximum(shift - 1, 0), 0)
    keep = keep + ((rem > half) | ((rem == half) & (shift > 0) & ((keep & 1) == 1))).astype(np.int64)
    carry = keep == (1 << (mb + 1))
    keep = np.where(carry, 1 << mb, keep)
    q = np.where(carry, q + 1, q)
    e_field = np.where(keep < (1 << mb), 0, q + mb + bias)
    big = e_field > (1 << eb) - 1                      # beyond every binade: saturate
    byte = np.where(big, top_byte, (np.clip(e_field, 0, (1 << eb) - 1) << mb) | (keep & ((1 << mb) - 1)))
    return np.minimum(byte, top_byte)


def dequantize(q, s, fmt):
    """fp32 [n]: decode(q) * 2^(s - 127) per block, one fp32 multiply per element."""
    q = np.asarray(q, dtype=np.uint8).reshape(-1)
    sf = np.repeat(decode_e8m0(s), BLOCK)[:q.size]
    with np.errstate(invalid="ignore", over="ignore"):
        return (decode(q, fmt) * sf).astype(np.float32)
