"""A numpy restatement of the MXFP4 format (OCP Microscaling v1.0: e2m1 elements, two per byte, one
E8M0 scale byte per 32) by integer bit manipulation: block quantisation, packing and dequantisation.
Independent of torch, of frexp / ldexp and of any floating-point operation but the contract's own
(one fp32 product per element in ``dequantize``)."""
import numpy as np

BLOCK = 32
EMAX = 2
# four times the seven midpoints between neighbouring e2m1 magnitudes (0.25 .. 5), and whether the tie
# goes up: to the neighbour whose mantissa bit is 0
MIDPOINTS_X4 = ((1, False), (3, True), (5, False), (7, True), (10, False), (14, True), (20, False))


def decode_e8m0(byte):
    b = np.asarray(byte, dtype=np.uint8).astype(np.int64)
    bits = np.where(b == 255, 0x7FC00000, np.where(b == 0, 0x00400000, b << 23))
    return bits.astype(np.uint32).view(np.float32)


def decode_e2m1(code):
    """fp32 value of each 4-bit code: sign, two exponent bits, one mantissa bit."""
    c = np.asarray(code).astype(np.int64)
    mag = c & 7
    # exponent field 0: 0 or 0.5; else 2^(ex - 1) * (1 + man / 2): fp32 exponent ex + 126, mantissa bit 22
    bits = np.where(mag == 0, 0, np.where(mag == 1, 0x3F000000, (mag + 252) << 22)) | ((c >> 3) & 1) << 31
    return bits.astype(np.uint32).view(np.float32)


def unpack(packed, n):
    """The n codes of the packed bytes: element 2i the low nibble of byte i, 2i + 1 the high one."""
    b = np.asarray(packed, dtype=np.uint8).reshape(-1)
    return np.stack([b & 15, b >> 4], axis=1).reshape(-1)[:n]


def pack(code):
    code = np.asarray(code, dtype=np.uint8).reshape(-1)
    if code.size % 2:
        code = np.concatenate([code, np.zeros(1, np.uint8)])        # the pad nibble is 0
    return (code[0::2] | (code[1::2] << 4)).astype(np.uint8)


def quantize_codes(x):
    """(codes [n], scale bytes [ceil(n / 32)]) of the flat fp32 array ``x``."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1))
    n = x.size
    nb = -(-n // BLOCK)
    u = np.zeros(nb * BLOCK, dtype=np.uint32)
    u[:n] = x.view(np.uint32)
    u = u.reshape(nb, BLOCK).astype(np.int64)
    mag = u & 0x7FFFFFFF
    is_nan, is_inf = mag > 0x7F800000, mag == 0x7F800000
    amax = np.where(mag < 0x7F800000, mag, 0).max(axis=1)       # bits order as magnitudes do
    ex = amax >> 23
    top_bit = np.floor(np.log2(np.maximum(amax & 0x7FFFFF, 1).astype(np.float64))).astype(np.int64)    # exact below 2^23
    fl = np.where(ex > 0, ex - 127, top_bit - 149)              # floor(log2 amax)
    e = np.where(amax == 0, 0, np.clip(fl - EMAX, -127, 127))
    scale_byte = np.where(is_nan.any(axis=1), 255, e + 127).astype(np.uint8)
    # |x| * 2^-e = sig * 2^(e2 - 23); four times that against the integer midpoints, exactly
    exf, man = mag >> 23, mag & 0x7FFFFF
    sig = np.where(exf == 0, man, man | 0x800000)
    sh = np.where(exf == 0, -126, exf - 127) - e[:, None] - 21  # 4 |x| 2^-e = sig * 2^sh
    up, down = np.clip(sh, 0, 8), np.clip(-sh, 0, 36)            # 2^8 sig > 20 for sig > 0; 2^36 > 2^24 * 20
    lhs = sig << up
    code = np.zeros(u.shape, dtype=np.int64)
    for t, tie_up in MIDPOINTS_X4:
        rhs = np.int64(t) << down
        code += (lhs >= rhs) if tie_up else (lhs > rhs)
    code = np.where(is_inf, 7, code)                            # saturating
    code = np.where(is_nan, 0, code | ((u >> 31) & 1) << 3)     # the sign is kept, -0 included; a NaN is code 0
    return code.reshape(-1)[:n].astype(np.uint8), scale_byte


def quantize(x):
    """(packed bytes [ceil(n / 2)], scale bytes [ceil(n / 32)])."""
    code, s = quantize_codes(x)
    return pack(code), s


def dequantize(packed, s, n):
    """fp32 [n]: decode_e2m1(code) * 2^(s - 127) per block, one fp32 multiply per element."""
    sf = np.repeat(decode_e8m0(s), BLOCK)[:n]
    with np.errstate(invalid="ignore", over="ignore"):
        return (decode_e2m1(unpack(packed, n)) * sf).astype(np.float32)
