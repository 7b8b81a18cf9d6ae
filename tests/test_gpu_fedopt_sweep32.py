"""GPU: the operand injection of tests/test_gpu_fedopt_sweep16.py for fp32 and fp64 keys.  These
dtypes cannot be swept exhaustively, so the operands are stratified.

fp32 (adapt_vec's flame_fm::sqrt_rn / div_rn and the general sequences of adapt_elem), BITWISE
against the C oracle:
  * v: every exponent field 0..255 x mantissas {0, 1, 0x400000, 0x7FFFFF, 12 seeded random}, the
    values 1 ulp either side of the admission bounds 2^-96 and 2^78, and negative values, under one
    ordinary m;
  * num: the same grid in both signs and 1 ulp either side of +-2^-85 and +-2^100, crossed with the
    256 v of fedopt_sweep.quotient_v_bits(float32) (+0, the subnormal ends, every binade up to 2^78);
  * tau at the fp32 admission bounds 2^-20 and 2^38, 1e-3 and 1 inside them, 2^-21 and 2^39 outside;
  * the three lane packings (lanes of 4), both layouts, both kernels.

fp64 (adapt_elem_f64's dsqrt_rn / ddiv_rn) against OracleFedOPT(sort, sqrt_rn=True) under the
comparison of test_gpu_fedopt_f64.py (sign bits compared, NaN equals NaN): the same mantissas over
every 8th exponent field of the 11, plus every exponent within 4 of 2^+-960, 2^-900, the subnormal
boundary and overflow, where ddiv_rn / dsqrt_rn switch behaviour; tau = 1e-3, 1, 2^-965 and 2^965
(the last two put den outside [2^-960, 2^960])."""
import functools
import itertools

import pytest
import torch

import fedopt_sweep as F

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
TAUS32 = {"lo": 2.0 ** -20, "1e-3": 1e-3, "one": 1.0, "hi": 2.0 ** 38, "under": 2.0 ** -21, "over": 2.0 ** 39}
TAUS64 = {"1e-3": 1e-3, "one": 1.0, "tiny": 2.0 ** -965, "huge": 2.0 ** 965}


def _around(bits):
    return [bits - 1, bits, bits + 1]


def _f32_bits(x):
    return int(torch.tensor(x, dtype=F32).view(torch.int32)) & 0xFFFFFFFF


@functools.lru_cache(maxsize=1)
def _source32():
    sign = 1 << 31
    grid = F.grid_bits(F32, range(256), seed=32)
    v = grid + _around(_f32_bits(2.0 ** -96)) + _around(_f32_bits(2.0 ** 78))
    v += [sign | b for b in (0, 1, _f32_bits(2.0 ** -100), _f32_bits(1.0), _f32_bits(2.0 ** 78), 0x7F800000)]
    num = grid + _around(_f32_bits(2.0 ** -85)) + _around(_f32_bits(2.0 ** 100))
    num += [sign | b for b in num]
    dens = F.quotient_v_bits(F32)
    m = torch.cat([torch.full((len(v),), F.M_ORDINARY), F.from_bits(num, F32).repeat(len(dens))])
    vv = torch.cat([F.from_bits(v, F32), F.from_bits(dens, F32).repeat_interleave(len(num))])
    return F.Source(F32, m, vv)


@functools.lru_cache(maxsize=1)
def _source64():
    near = [1023 + 960, 1023 - 960, 1023 - 900, 0, 2047]
    exps = sorted(set(range(0, 2048, 8)) | {e + k for e in near for k in range(-4, 5) if 0 <= e + k <= 2047})
    sign = 1 << 63
    grid = F.grid_bits(F64, exps, seed=64)
    v = grid + [sign | b for b in (0, 1, 1023 << 52, 2046 << 52, 2047 << 52)]
    num = grid + [sign | b for b in grid]
    ones = (1 << 52) - 1
    dens = [(e << 52) | mant for e in exps[::3] if e < 2047 for mant in (0, ones)]
    m = torch.cat([torch.full((len(v),), F.M_ORDINARY, dtype=F64), F.from_bits(num, F64).repeat(len(dens))])
    vv = torch.cat([F.from_bits(v, F64), F.from_bits(dens, F64).repeat_interleave(len(num))])
    return F.Source(F64, m, vv)


@functools.lru_cache(maxsize=1)
def _expected_cached(dt, sort, tau):
    src = _source32() if dt == "f32" else _source64()
    return tuple(t.to(DEV) for t in F.oracle_collapsed(sort, tau, src, sqrt_rn=dt == "f64"))


def _expected(dt, sort, tau):
    from oracle import consult
    consult.note()      # every case compares with the oracle's results, whichever case computed them
    return _expected_cached(dt, sort, tau)


def _required(src):
    """The entries whose current' is a number: m not NaN, v not NaN and not negative (-0 is not)."""
    m, v = src.m[:src.n], src.v[:src.n]
    return ~torch.isnan(m) & ~torch.isnan(v) & ~(v < 0)


@pytest.mark.parametrize("sort,tau,packing,layout,kernel", [
    pytest.param(*c, id="-".join(c)) for c in itertools.product(F.SORTS, TAUS32, F.PACKINGS, F.LAYOUTS, F.KERNELS)])
def test_fp32_sweep(sort, tau, packing, layout, kernel):
    t = TAUS32[tau]
    src = _source32()
    masks = F.run_case(f"f32/{sort}", sort, F.collapse_hyper(sort, t), kernel, layout, packing, src,
                       _expected("f32", sort, t), DEV)
    required = _required(src)
    print(f"f32/{sort}/tau={t}/{packing}/{layout}/{kernel}: {int(masks['current'].sum())} of {src.n} compared "
          f"bitwise, {int(required.sum())} required")
    assert int(required.sum()) > src.n // 3 and bool(masks["current"][required].all())
    assert bool(masks["m"][~torch.isnan(src.m[:src.n])].all()) and bool(masks["v"][~torch.isnan(src.v[:src.n])].all())


@pytest.mark.filterwarnings("ignore:overflow encountered in cast:RuntimeWarning")   # tau = 2^965 as an fp32 scalar: unused by fp64 keys
@pytest.mark.parametrize("sort,tau,layout,kernel", [
    pytest.param(*c, id="-".join(c)) for c in itertools.product(F.SORTS, TAUS64, F.LAYOUTS, F.KERNELS)])
def test_fp64_sweep(sort, tau, layout, kernel):
    """fp64 has no admission: one packing.  Bitwise on every element that is not NaN on both sides is
    test_gpu_fedopt_f64.py's comparison (values equal and sign bits equal)."""
    t = TAUS64[tau]
    src = _source64()
    masks = F.run_case(f"f64/{sort}", sort, F.collapse_hyper(sort, t), kernel, layout, "pure", src,
                       _expected("f64", sort, t), DEV)
    required = _required(src)
    print(f"f64/{sort}/tau={t}/{layout}/{kernel}: {int(masks['current'].sum())} of {src.n} compared bitwise, "
          f"{int(required.sum())} required")
    assert int(required.sum()) > src.n // 3 and bool(masks["current"][required].all())
